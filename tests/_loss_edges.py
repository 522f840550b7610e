"""Named edge cases of the ground-truth encoding (csrc/train_kernels.hip `encode_gt_*_kernel`, lib_yolo/tfdata.py:77-171) and of
the training loss (`loss_kernel`, lib_yolo/layers.py:126-188), built deterministically.  No tests here: tests/test_loss_edges_cpu.py,
tests/test_loss_edges_gpu.py and oracle/make_golden_loss_edges.py import the same inputs from this module.

Encode cases: dict(name, layers [(h, w, [(prior_h, prior_w)] * 3)], boxes [B, M, 4] float32, labels [B, M] int32, counts [B] int32 or
None, ign_thresh, check).  `check(case, enc)` asserts the property that defines the case on the FLOAT32 oracle's output (`enc[i]` =
oracle.train_ref.encode_boxes of image i), so that a case cannot go vacuous unnoticed.  Finite inputs only, and no box with
prior_area + box_area == 0: what a NaN IoU does to the maximum is not what these cases pin.

Loss cases: dict(name, raw [S, lh, lw, F] float32, gt {loc, obj, cls, ign}, C, aleatoric, aleatoric_loss, planted), `planted` = the
indices (s, row, col, box) of the prior boxes that carry the planted values."""
import functools
import hashlib
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
IGN = 0.7
F32 = np.float32
LOGIT_LO, LOGIT_HI = -np.log(1 / F32(1e-7) - 1), -np.log(1 / F32(1 - 1e-7) - 1)      # logit(1e-7), logit(1 - 1e-7): -16.118, +15.942


def ecp_layers(hw, table="ECP_9_PRIORS"):
    pri = json.load(open(os.path.join(GOLDEN, "priors.json")))[table]
    return [(int(hw[0]) // s, int(hw[1]) // s, [tuple(p) for p in pri[str(s)]]) for s in (32, 16, 8)]


def n_priors(layers):
    return sum(h * w * len(p) for h, w, p in layers)


def image_boxes(case, i):
    """The boxes and labels of image i that count: `counts` clamped to [0, M] like the kernel (and like a dataset that pads)."""
    m = case["boxes"].shape[1]
    n = m if case["counts"] is None else min(max(int(case["counts"][i]), 0), m)
    return case["boxes"][i, :n], case["labels"][i, :n]


def oracle_encode(case, dtype=np.float32):
    from oracle import train_ref
    return [train_ref.encode_boxes(*image_boxes(case, i), case["layers"], case["ign_thresh"], dtype=dtype) for i in range(case["boxes"].shape[0])]


def ious(case, box):
    """float32 IoU of one box with every prior box (all layers back to back), and the in-cell mask of tfdata.py:114-118."""
    from oracle import train_ref
    pd = train_ref.prior_data(case["layers"], np.float32)
    b = np.asarray(box, np.float32)
    x, y = (b[3] + b[1]) / F32(2), (b[2] + b[0]) / F32(2)
    dx, dy = pd["lw"] * (x - pd["cx"]), pd["lh"] * (y - pd["cy"])
    return train_ref.calc_iou(b, pd), (dx >= 0) & (dx <= 1) & (dy >= 0) & (dy <= 1)


def _flat(enc, name):
    return np.concatenate([e[name].reshape(-1, 4) if name == "loc" else e[name].reshape(-1) for e in enc])


def _case(name, layers, boxes, labels, check, counts=None, ign_thresh=IGN):
    boxes = np.asarray(boxes, np.float32)
    labels = np.asarray(labels, np.int32)
    if boxes.ndim == 2:
        boxes, labels = boxes[None], labels[None]
    assert np.isfinite(boxes).all()
    return {"name": name, "layers": layers, "boxes": np.ascontiguousarray(boxes), "labels": np.ascontiguousarray(labels),
            "counts": None if counts is None else np.asarray(counts, np.int32), "ign_thresh": float(ign_thresh), "check": check}


def _centred(cy, cx, h, w):
    return [cy - h / 2, cx - w / 2, cy + h / 2, cx + w / 2]


# ---------------------------------------------------------------------------------------------------------------------
# encode cases
# ---------------------------------------------------------------------------------------------------------------------
def _tie_cases():
    """64 x 128: grids 2 x 4, 4 x 8, 8 x 16 -- col / lw, row / lh and the dyadic box coordinates are exact in float32.  Two neighbours'
    IoUs are the SAME float32 number by construction, not by luck:
      across a vertical border (x = 0.75) the prior boxes of columns 2 and 3 lie in [0.5, 1), where float32 is a uniform grid of
        which the column pitch is a multiple, so they are exact translates; the box contains both in x;
      across the horizontal border (y = 0.5) the stride-32 priors are taller than a cell, the two rows' prior boxes overlap, and the
        box lies inside both in y: the intersection's height is the box's own.
    The cell left of (above) the border has d = 1 -> clipped to 1 - 1e-7, the other d = 0 -> clipped to 1e-7; logit of either needs
    the IEEE division 1 / x."""
    L = ecp_layers((64, 128))
    out = []
    for kind, box, cells in (("vertical", [0.0625, 0.5, 0.3125, 1.0], 2),              # centre (0.1875, 0.75): inside a row of every layer
                             ("horizontal", [0.46875, 0.625, 0.53125, 0.6875], 2),      # centre (0.5, 0.65625): inside a column of every layer
                             ("corner", [0.46875, 0.5, 0.53125, 1.0], 4)):              # centre (0.5, 0.75)
        def check(case, enc, kind=kind, cells=cells):
            iou, cell = ious(case, case["boxes"][0, 0])
            obj, loc = _flat(enc[0], "obj"), _flat(enc[0], "loc")
            won = (iou >= iou.max()) & cell
            assert iou.max() > 0 and won.sum() >= 2, "exact tie: two or more object prior boxes with IoU > 0"
            assert np.array_equal(obj > 0, won) and int(obj.sum()) == cells, "objects: %d, cells wanted: %d" % (obj.sum(), cells)
            lx, ly = loc[obj > 0, 0], loc[obj > 0, 1]
            lo, hi = np.isclose([lx, ly], LOGIT_LO, rtol=1e-6), np.isclose([lx, ly], LOGIT_HI, rtol=1e-6)
            if kind in ("vertical", "corner"):
                assert lo[0].sum() == cells // 2 and hi[0].sum() == cells // 2, "loc_x: logit(1e-7) right of the border, logit(1 - 1e-7) left of it"
            if kind in ("horizontal", "corner"):
                assert lo[1].sum() == cells // 2 and hi[1].sum() == cells // 2, "loc_y likewise"
        out.append(_case("tie_on_border_" + kind, L, [box], [1], check))
    return out


def _all_iou_zero():
    L = ecp_layers((64, 128))
    ph, pw = L[2][2][1]

    def check(case, enc):
        iou, _ = ious(case, case["boxes"][0, 0])
        assert iou.max() == 0 and (iou == 0).all()
        assert [int(e["obj"].sum()) for e in enc[0]] == [12, 12, 12]
        assert all((e["ign"] == 1).all() for e in enc[0])
    return [_case("all_iou_zero", L, [_centred(0.5, 0.5, ph, pw)], [1], check)]


def _degenerate_boxes():
    L = ecp_layers((64, 128))
    ph, pw = L[1][2][0]

    def check_zero(case, enc):
        iou, _ = ious(case, case["boxes"][0, 0])
        assert (iou == 0).all() and not np.signbit(iou).any()
        obj, loc = _flat(enc[0], "obj"), _flat(enc[0], "loc")
        assert obj.sum() >= 3 and (loc[obj > 0, 2] == np.log(F32(1e-7))).all(), "loc_w = log(1e-7) on every object"

    def check_inv(case, enc):
        iou, _ = ious(case, case["boxes"][0, 0])
        assert (iou == 0).all() and np.signbit(iou).any(), "IoU = +-0 everywhere, -0 somewhere"
        obj, loc = _flat(enc[0], "obj"), _flat(enc[0], "loc")
        assert obj.sum() >= 3 and (loc[obj > 0, 3] == np.log(F32(1e-7))).all()
    # centres inside a cell of every layer (0.3, 0.3): not on a border
    return [_case("zero_area", L, [[0.3 - ph / 2, 0.3, 0.3 + ph / 2, 0.3]], [1], check_zero),
            _case("inverted", L, [[0.3 + ph / 2, 0.3 - pw / 2, 0.3 - ph / 2, 0.3 + pw / 2]], [0], check_inv)]


def _image_edges():
    L = ecp_layers((608, 608))
    (ph0, pw0), (ph1, pw1), (ph2, pw2) = L[0][2][0], L[1][2][1], L[2][2][2]
    boxes = [_centred(0.0, 0.0, ph0, pw0), _centred(1.0, 1.0, ph0, pw0), _centred(0.0, 1.0, ph1, pw1), _centred(1.0, 0.0, ph2, pw2),
             _centred(1.0, 1.0, ph1, pw1), _centred(1.0, 1.0, ph2, pw2), [-0.1, -0.2, 1.1, 1.3]]
    labels = [0, 1, 1, 0, 1, 0, 1]

    def check(case, enc):
        bb = case["boxes"][0]
        assert (bb < 0).any() and (bb > 1).any() and ((bb[:, 2] - bb[:, 0]) * (bb[:, 3] - bb[:, 1]) > 1).any()
        assert enc[0][0]["obj"][0, 0].sum() == 1, "the box centred on (0, 0) finds its prior box in cell (0, 0)"
        # d of the last column (row) at x = 1 (y = 1): lw * (1 - (lw - 1) / lw) in float32 is below 1 on 19 x 19 -- the box centred on (1, 1)
        # is an object of cell (18, 18) -- and above 1 on 38 x 38 and 76 x 76, where the boxes centred on an edge are nobody's
        last = [float(F32(lw) * (F32(1) - F32((lw - 1) / float(lw)))) for _, lw, _ in case["layers"]]
        assert last[0] <= 1 and last[1] > 1 and last[2] > 1, last
        assert enc[0][0]["obj"][18, 18].sum() == 1 and [int(e["obj"].sum()) for e in enc[0]] == [2, 0, 0]
    return [_case("image_edges", L, boxes, labels, check)]


def _overwrite():
    L = ecp_layers((608, 608))
    ph, pw = L[1][2][0]
    cy, cx = 10.5 / 38, 20.5 / 38                                    # the middle of cell (10, 20) of layer 1
    a = _centred(cy, cx, ph, pw)
    b = _centred(cy, cx, ph * 1.1, pw * 0.9)                        # same cell, same best prior box, other size
    ph0, pw0 = L[0][2][0]
    # the stride-32 prior's shape with its centre just above the image: IoU 0.9 with row 0's prior box, but no cell has 0 <= d_y <= 1
    skipped = _centred(-1e-4, 4.5 / 19, ph0, pw0)

    def check(case, enc):
        bb = case["boxes"][0]
        assert np.array_equal(bb[0], bb[2]) and not np.array_equal(bb[0], bb[1])
        won = [(i >= i.max()) & c for i, c in (ious(case, bb[j]) for j in range(3))]
        assert all(w.sum() == 1 for w in won) and np.array_equal(won[0], won[1]), "three boxes, one prior box"
        n = int(np.flatnonzero(won[0])[0])
        cls, loc, obj, ign = (_flat(enc[0], k) for k in ("cls", "loc", "obj", "ign"))
        from oracle import train_ref
        alone = train_ref.encode_boxes(bb[:1], case["labels"][0, :1], case["layers"], case["ign_thresh"])
        middle = train_ref.encode_boxes(bb[1:2], case["labels"][0, 1:2], case["layers"], case["ign_thresh"])
        assert cls[n] == 0 and np.array_equal(loc[n], _flat(alone, "loc")[n]) and not np.array_equal(loc[n], _flat(middle, "loc")[n]), "the last wins"
        assert _flat(middle, "cls")[n] == 1
        iou, cell = ious(case, bb[3])
        assert not ((iou >= iou.max()) & cell).any(), "the fourth box's best prior box is not in a cell that claims its centre"
        hit = iou >= F32(case["ign_thresh"])
        assert hit.sum() >= 1 and (ign[hit] == 0).all() and (obj[hit] == 0).all(), "... it sets no object but zeroes ign"
        assert obj.sum() == 1
    return [_case("overwrite", L, [a, b, a, skipped], [0, 1, 0, 1], check)]


def _ign_extremes():
    from oracle import train_ref
    L = ecp_layers((64, 128))
    ph, pw = L[1][2][1]
    boxes = [_centred(0.3, 0.3, ph, pw), _centred(0.7, 0.6, ph * 1.2, pw)]

    def check0(case, enc):
        obj, ign = _flat(enc[0], "obj"), _flat(enc[0], "ign")
        assert obj.sum() == 2 and np.array_equal(ign, obj), "ign_thresh = 0: every IoU >= 0, ign survives on the objects only"
    # ign_thresh = 1: a box EQUAL to a prior box, the first whose float32 IoU with itself is exactly 1
    pd = train_ref.prior_data(L, np.float32)
    case1 = _case("ign_thresh_one", L, np.zeros((1, 4)), [1], None, ign_thresh=1.0)
    for n in range(pd["bboxes"].shape[0]):
        iou, _ = ious(case1, pd["bboxes"][n])
        if iou[n] == 1:
            break
    else:
        raise AssertionError("no prior box with IoU exactly 1 with itself")
    near = pd["bboxes"][n] + F32(1e-4) * np.asarray([1, 1, 1, 1], np.float32)        # the same box shifted: IoU just below 1

    def check1(case, enc, n=n):
        iou, _ = ious(case, case["boxes"][0, 0])
        assert iou[n] == 1 and (iou >= 1).sum() == 1
        near_iou, _ = ious(case, case["boxes"][0, 1])
        assert 0.9 < near_iou.max() < 1
        assert _flat(enc[0], "obj")[n] == 1 and (_flat(enc[0], "ign") == 1).all(), "IoU 1 only on the object, ign = max(0, 1); nothing else reaches 1"
    return [_case("ign_thresh_zero", L, boxes, [1, 0], check0, ign_thresh=0.0),
            _case("ign_thresh_one", L, [pd["bboxes"][n], near], [1, 0], check1, ign_thresh=1.0)]


def fused_ious(case, box):
    """What calc_iou gives in float32 if the compiler contracts it into fused multiply-adds: (a) only the union's
    `+ box_h * box_w`, (b) only `area - h * w`, (c) both.  Emulated in float64, where a product of two float32 is exact."""
    from oracle import train_ref
    pd = train_ref.prior_data(case["layers"], np.float32)
    bb, b = pd["bboxes"], np.asarray(box, np.float32)
    h = np.maximum(np.minimum(bb[:, 2], b[2]) - np.maximum(bb[:, 0], b[0]), F32(0))
    w = np.maximum(np.minimum(bb[:, 3], b[3]) - np.maximum(bb[:, 1], b[1]), F32(0))
    inter, bh, bw = h * w, b[2] - b[0], b[3] - b[1]
    area = pd["bbox_areas"]
    plain = area - inter
    fused = (area.astype(np.float64) - h.astype(np.float64) * w.astype(np.float64)).astype(np.float32)
    out = []
    for sub, add_fused in ((plain, True), (fused, False), (fused, True)):
        union = (sub.astype(np.float64) + np.float64(bh) * np.float64(bw)).astype(np.float32) if add_fused else sub + bh * bw
        out.append(inter / union)
    return out


def _ign_thresh_equal():
    """ign_thresh EQUAL to the float32 IoU of a prior box that is no object: `iou >= ign_thresh` holds with equality and zeroes ign
    there; `>` would not.  The box is the first of a seeded sequence for which every fused form of calc_iou rounds that IoU lower,
    so a build whose calc_iou is contracted into fused multiply-adds leaves ign at 1 on that prior box.  (Today's compiler packs the
    two products of calc_iou into one instruction before it would contract them, so dropping `fp contract(off)` alone changes no
    mask; an explicitly fused union does fail this case.)"""
    L = ecp_layers((64, 128))
    rng = np.random.default_rng(16)
    probe = _case("ign_thresh_equal", L, np.zeros((1, 4)), [1], None)
    for _ in range(2000):
        box = np.asarray(_prior_shaped_boxes(rng, L, 1)[0], np.float32)
        iou, cell = ious(probe, box)
        cand = np.flatnonzero((iou > 0.2) & (iou < iou.max()) & ~((iou >= iou.max()) & cell))
        fused = fused_ious(probe, box)
        cand = [n for n in cand if all(f[n] < iou[n] for f in fused)]
        if cand:
            n = int(cand[0])
            break
    else:
        raise AssertionError("no box found")
    thresh = float(iou[n])

    def check(case, enc, n=n):
        iou, _ = ious(case, case["boxes"][0, 0])
        assert F32(case["ign_thresh"]) == iou[n] and 0.2 < iou[n] < iou.max()
        assert all(f[n] < iou[n] for f in fused_ious(case, case["boxes"][0, 0])), "every fused form is below the threshold"
        assert _flat(enc[0], "obj")[n] == 0 and _flat(enc[0], "ign")[n] == 0 and _flat(enc[0], "obj").sum() >= 1
    return [_case("ign_thresh_equal", L, [box], [1], check, ign_thresh=thresh)]


def _tiny_layers(which):
    return {1: [(1, 1, [(0.8, 0.7), (0.5, 0.4), (0.3, 0.6)])],
            3: [(1, 1, [(0.8, 0.7), (0.5, 0.4), (0.3, 0.6)]), (2, 2, [(0.45, 0.35), (0.3, 0.4), (0.25, 0.2)]),
                (4, 4, [(0.2, 0.15), (0.12, 0.2), (0.1, 0.08)])],
            4: [(1, 2, [(0.8, 0.45), (0.5, 0.3), (0.6, 0.4)]), (2, 3, [(0.45, 0.3), (0.3, 0.25), (0.35, 0.2)]),
                (3, 5, [(0.3, 0.18), (0.2, 0.15), (0.25, 0.1)]), (5, 7, [(0.15, 0.1), (0.1, 0.12), (0.08, 0.06)])]}[which]


def _prior_shaped_boxes(rng, layers, n, lo=0.02, hi=0.98):
    flat = [p for l in layers for p in l[2]]
    bb = np.zeros((n, 4), np.float32)
    for j in range(n):
        ph, pw = flat[rng.integers(len(flat))]
        bb[j] = _centred(rng.uniform(lo, hi), rng.uniform(lo, hi), ph * rng.uniform(0.8, 1.25), pw * rng.uniform(0.8, 1.25))
    return bb


def _tiny_and_layers():
    out = []
    for which, total in ((1, 3), (3, 63), (4, 174)):
        L = _tiny_layers(which)
        rng = np.random.default_rng(100 + which)
        # one box of every prior's own shape in the middle of some cell of its layer (so that every layer gets objects), then a few random ones
        bb = [_centred((rng.integers(h) + 0.5) / h, (rng.integers(w) + 0.5) / w, p[0], p[1]) for h, w, pri in L for p in pri[:2]]
        bb = np.concatenate([np.asarray(bb, np.float32), _prior_shaped_boxes(rng, L, 3)])
        lab = rng.integers(0, 3, bb.shape[0])

        def check(case, enc, total=total):
            assert n_priors(case["layers"]) == total and len(enc[0]) == len(case["layers"])
            assert all(e["obj"].sum() >= 1 for e in enc[0]), "every layer has an object"
        out.append(_case("layers_%d" % which, L, bb, lab, check))
    return out


def _counts():
    L = ecp_layers((64, 96))
    rng = np.random.default_rng(7)
    m = 4
    bb = (rng.uniform(-1e3, 1e3, (4, m, 4))).astype(np.float32)      # padding rows: finite garbage
    lab = rng.integers(-50, 50, (4, m)).astype(np.int32)
    bb[0] = _prior_shaped_boxes(rng, L, m); lab[0] = [1, 0, 1, 1]
    bb[3, 0] = _prior_shaped_boxes(rng, L, 1)[0]; lab[3, 0] = 1

    def check(case, enc):
        assert case["counts"].tolist() == [case["boxes"].shape[1] + 5, -3, 0, 1]
        objs = [sum(int(e["obj"].sum()) for e in img) for img in enc]
        assert objs[0] >= 3 and objs[1] == 0 and objs[2] == 0 and objs[3] == 1
        for img in enc[1:3]:
            assert all((e["ign"] == 1).all() and (e["loc"] == 0).all() and (e["cls"] == 0).all() for e in img)

    def check_none(case, enc):
        assert case["boxes"].shape[1] == 0
        for img in enc:
            assert all((e["ign"] == 1).all() and (e["loc"] == 0).all() and (e["cls"] == 0).all() and (e["obj"] == 0).all() for e in img)
    return [_case("counts", L, bb, lab, check, counts=[m + 5, -3, 0, 1]),
            _case("no_boxes", L, np.zeros((2, 0, 4), np.float32), np.zeros((2, 0), np.int32), check_none)]


def _many_images():
    L = _tiny_layers(3)
    rng = np.random.default_rng(300)
    B, m = 300, 5
    counts = rng.integers(0, m + 1, B).astype(np.int32)
    bb = rng.uniform(-1e3, 1e3, (B, m, 4)).astype(np.float32)
    lab = rng.integers(0, 3, (B, m)).astype(np.int32)
    for i in range(B):
        bb[i, :counts[i]] = _prior_shaped_boxes(rng, L, int(counts[i]))

    def check(case, enc):
        assert len(enc) == 300 and sorted(set(case["counts"].tolist())) == [0, 1, 2, 3, 4, 5]
        objs = np.asarray([sum(int(e["obj"].sum()) for e in img) for img in enc])
        assert (objs[case["counts"] == 0] == 0).all() and (objs[case["counts"] > 0] >= 1).all()
        assert len({tuple(_flat(img, "obj").tolist()) for img in enc}) > 100, "the images differ"
    return [_case("many_images", L, bb, lab, check, counts=counts)]


@functools.lru_cache(maxsize=None)
def encode_cases():
    """Every encode case, built once per process: treat the arrays as read-only."""
    return _tie_cases() + _all_iou_zero() + _degenerate_boxes() + _image_edges() + _overwrite() + _ign_extremes() + _ign_thresh_equal() + _counts() + \
        _tiny_and_layers() + _many_images()


# ---------------------------------------------------------------------------------------------------------------------
# loss cases
# ---------------------------------------------------------------------------------------------------------------------
def block(C, aleatoric):
    return (10 + 2 * C) if aleatoric else (5 + C)


def _loss_base(seed, S, lh, lw, C, aleatoric, aleatoric_loss, obj_frac=0.3, sigma=1.5):
    """Moderate N(0, sigma) logits; gt.loc within 1.9 of the predicted loc (|gt.loc - loc| <= 2: (d * d) * exp(40) stays in float32);
    objects at `obj_frac`; ign = 1 on objects and on about 4 of 5 others."""
    rng = np.random.default_rng(seed)
    blk = block(C, aleatoric)
    raw = (rng.standard_normal((S, lh, lw, 3 * blk)) * sigma).astype(np.float32)
    r = raw.reshape(S, lh, lw, 3, blk)
    gt = {"loc": (r[..., 0:4] + rng.uniform(-1.9, 1.9, (S, lh, lw, 3, 4))).astype(np.float32),
          "obj": (rng.random((S, lh, lw, 3)) < obj_frac).astype(np.float32),
          "cls": rng.integers(0, C, (S, lh, lw, 3)).astype(np.int32)}
    gt["ign"] = np.maximum(gt["obj"], (rng.random((S, lh, lw, 3)) < 0.8).astype(np.float32))
    return rng, raw, r, gt


def _loss_case(name, raw, gt, C, aleatoric, aleatoric_loss, planted=()):
    assert np.isfinite(raw).all()
    return {"name": name, "raw": np.ascontiguousarray(raw), "gt": {k: np.ascontiguousarray(v) for k, v in gt.items()}, "C": C,
            "aleatoric": aleatoric, "aleatoric_loss": aleatoric_loss, "planted": [tuple(int(v) for v in p) for p in planted]}


def _priors_of(shape):
    return [tuple(i) for i in np.ndindex(*shape)]


CLIP_HI = [40.0, float(np.nextafter(F32(40), F32(np.inf))), 39.999, 100.0, 1e4]
CLIP_LO = [-v for v in CLIP_HI]


def clip(side, C=2, aleatoric_loss=True):
    """Log variances on and around the clip at +-40 (lib_yolo/layers.py:151), on OBJECT prior boxes with ign mixed.  The two sides
    live in two tensors: exp(40) * d * d ~ 1e17 would make every other term of the sum invisible."""
    S, lh, lw = 2, 3, 4
    rng, raw, r, gt = _loss_base(40 + (side == "lo") + 10 * C, S, lh, lw, C, True, aleatoric_loss)
    vals = CLIP_HI if side == "hi" else CLIP_LO
    idx = _priors_of((S, lh, lw, 3))[::3]                             # every third prior box: 24 of 72
    for j, p in enumerate(idx):
        for k in range(4):
            r[p][4 + k] = vals[(j + k) % len(vals)]                  # every value meets every coordinate
        gt["obj"][p] = 1
        gt["ign"][p] = 1 if j % 2 else gt["ign"][p]
    gt["ign"] = np.maximum(gt["ign"], gt["obj"])
    return _loss_case("clip_%s%s%s" % (side, "" if aleatoric_loss else "_plain", "" if C == 2 else "_c%d" % C), raw, gt, C, True, aleatoric_loss, idx)


SAT_OBJ = [0.0, 17.0, -17.0, 30.0, -30.0, 88.8, -88.8, 90.0, -90.0, -103.9, 1e4, -1e4]


def saturated_obj(C=2, aleatoric=True):
    """Objectness logits where expf(-x) overflows (x < -88.72), where expf(-|x|) is denormal or 0, and where sigmoid rounds to 0 / 1;
    each on an object, on a non-object that counts (ign = 1) and on an ignored prior box (ign = 0)."""
    S, lh, lw = 2, 3, 4
    rng, raw, r, gt = _loss_base(60 + 10 * C + aleatoric, S, lh, lw, C, aleatoric, aleatoric)
    idx = _priors_of((S, lh, lw, 3))[:3 * len(SAT_OBJ)]
    o = 8 if aleatoric else 4
    for j, p in enumerate(idx):
        r[p][o] = SAT_OBJ[j % len(SAT_OBJ)]
        kind = j // len(SAT_OBJ)
        gt["obj"][p], gt["ign"][p] = (1, 1) if kind == 0 else ((0, 1) if kind == 1 else (0, 0))
    return _loss_case("saturated_obj_%s_c%d" % ("ale" if aleatoric else "std", C), raw, gt, C, aleatoric, aleatoric, idx)


def class_spread(C, aleatoric=True):
    """Class logits from {-100, 0, 100} (expf(x - lse) underflows), all equal, or the label on the smallest logit; every prior box
    an object.  C = 1: lse = x, loss and gradient exactly 0."""
    S, lh, lw = 2, 3, 4
    rng, raw, r, gt = _loss_base(80 + 10 * C + aleatoric, S, lh, lw, C, aleatoric, aleatoric)
    idx = _priors_of((S, lh, lw, 3))
    c0 = 10 if aleatoric else 5
    for j, p in enumerate(idx):
        kind = j % 3
        if kind == 0:
            r[p][c0:c0 + C] = rng.choice([-100.0, 0.0, 100.0], C)
        elif kind == 1:
            r[p][c0:c0 + C] = [-100.0, 0.0, 100.0, 3.5][(j // 3) % 4]
        else:
            r[p][c0:c0 + C] = rng.choice([-100.0, 0.0, 100.0], C) + rng.standard_normal(C)
            gt["cls"][p] = int(np.argmin(r[p][c0:c0 + C]))
        gt["obj"][p] = 1
        gt["ign"][p] = 1
    return _loss_case("class_spread_%s_c%d" % ("ale" if aleatoric else "std", C), raw, gt, C, aleatoric, aleatoric, idx)


def wrap():
    """S * lh * lw * 3 = 263 160 > LOSS_MAX_BLOCKS * 256 = 262 144: 1028 workgroups' worth of prior boxes on 1024, the last 1016
    prior boxes are the grid-stride loop's second trip."""
    S, lh, lw, C = 3, 172, 170, 2
    rng, raw, r, gt = _loss_base(1028, S, lh, lw, C, True, True, obj_frac=0.05)
    assert S * lh * lw * 3 == 263160
    return _loss_case("wrap", raw, gt, C, True, True)


def one_cell(lw):
    """S = 1 on a 1 x 1 grid (3 threads) or a 1 x 22 grid (66 threads: a full wave and two lanes)."""
    rng, raw, r, gt = _loss_base(200 + lw, 1, 1, lw, 2, True, True, obj_frac=0.5)
    gt["obj"][0, 0, 0, 0] = 1; gt["obj"][0, 0, -1, 2] = 1
    gt["ign"] = np.maximum(gt["ign"], gt["obj"])
    return _loss_case("one_cell_1x%d" % lw, raw, gt, 2, True, True)


def layout():
    """S = 2, 5 x 7, C = 5: the dense tensors; the test spreads them to pitch = F + 2, grad_pitch = F + 6, gt_stride = lh * lw * 3 + 40."""
    rng, raw, r, gt = _loss_base(57, 2, 5, 7, 5, True, True)
    return _loss_case("layout", raw, gt, 5, True, True)


CLASS_COUNTS = (1, 2, 3, 80, 128)


@functools.lru_cache(maxsize=None)
def loss_cases(big=True):
    """Every loss case (big: with `wrap`), built once per process: treat the arrays as read-only."""
    out = [clip("hi"), clip("lo"), clip("hi", aleatoric_loss=False), clip("lo", aleatoric_loss=False), saturated_obj()]
    out += [class_spread(C) for C in CLASS_COUNTS]
    out += [f(C, aleatoric=False) for C in (2, 80) for f in (saturated_obj, class_spread)]
    out += [one_cell(1), one_cell(22), layout()]
    return out + ([wrap()] if big else [])


def derivative_cases():
    """clip, saturated_obj and class_spread at C = 3, for the central differences of the float64 oracle."""
    return [clip("hi", C=3), clip("lo", C=3), saturated_obj(C=3), class_spread(3)]


# ---------------------------------------------------------------------------------------------------------------------
# bounds (tests/test_loss_edges_cpu.py's docstring derives them) and the fixture's input hash
# ---------------------------------------------------------------------------------------------------------------------
def reference_loss(case, dtype=np.float64, want_grad=True):
    from oracle import train_ref
    with np.errstate(over="ignore"):                                   # exp(1e4) = inf -> sigmoid 0: the documented formula, and IEEE
        return train_ref.loss(case["raw"], case["gt"], case["C"], case["aleatoric"], case["aleatoric_loss"], dtype=dtype, want_grad=want_grad,
                              want_abs=True)


def sum_bounds(ref):
    """1e-5 * max(1, A) per sum, A = the float64 sum of the ABSOLUTE per-prior-box terms over the sum's own divisor."""
    return {k: 1e-5 * max(1.0, float(ref["abs"][k])) for k in ("loc", "obj", "cls")}


def distances(got_sums, got_grad, ref):
    """Worst distance of the three sums and of the gradient elements from the float64 reference, as fractions of their bounds
    (gradient elements: 1e-5 * max(1, |ref|))."""
    b = sum_bounds(ref)
    out = {k: abs(float(got_sums[i]) - float(ref[k])) / b[k] for i, k in enumerate(("loc", "obj", "cls"))}
    if got_grad is not None:
        g = np.asarray(ref["grad"], np.float64)
        out["grad"] = float((np.abs(np.asarray(got_grad, np.float64) - g) / (1e-5 * np.maximum(1.0, np.abs(g)))).max())
    return out


def input_hash(case):
    h = hashlib.sha256()
    arrays = [case["boxes"], case["labels"]] if "boxes" in case else [case["raw"]] + [case["gt"][k] for k in ("loc", "obj", "cls", "ign")]
    if case.get("counts") is not None:
        arrays.append(case["counts"])
    if "layers" in case:
        arrays.append(np.asarray([[h_, w_] + [v for p in pri for v in p] for h_, w_, pri in case["layers"]], np.float64))
        arrays.append(np.asarray([case["ign_thresh"]], np.float64))
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(("%s%s" % (a.dtype.str, a.shape)).encode())
        h.update(a.tobytes())
    return h.hexdigest()
