"""Ground-truth encoding and the training loss at their edges (csrc/train_kernels.hip), the part that runs anywhere: the cases of
tests/_loss_edges.py are what they claim to be, the float32 restatement reaches the bounds the device is held to, the analytic
gradient is the derivative at the planted values, and the restatement equals the reference's own functions on these inputs
(tests/golden/loss_edges.npz, oracle/make_golden_loss_edges.py).  The device part is tests/test_loss_edges_gpu.py.

Bounds (shared with the device part through _loss_edges.distances), derived, not tuned:
  gradient elements   1e-5 * max(1, |ref|), the bound of tests/test_loss.py
  the three sums      1e-5 * max(1, A), A = the float64 sum of the ABSOLUTE per-prior-box terms over the sum's divisor (2 S for loc,
                      S for obj and cls).  A float32 implementation rounds each term in float32 -- a handful of operations at 2^-24
                      each and an expf / logf / log1pf of a few ulp: well under 1e-6 of the term's operands -- and sums in double, so
                      its error is about 1e-6 * A; 1e-5 leaves a decade.  A and not |ref|: log-variance terms of both signs cancel in
                      the loc sum.  Where nothing cancels A == |ref| and this is the bound of tests/test_loss.py."""
import numpy as np
import pytest

import _loss_edges as E
from conftest import golden, assert_close

ENCODE = E.encode_cases()
LOSS = E.loss_cases()
DERIV = E.derivative_cases()
_name = lambda c: c["name"]


@pytest.fixture(scope="module")
def oracle_encoded():
    return {c["name"]: E.oracle_encode(c) for c in ENCODE}


def test_the_cases_are_all_there():
    names = [c["name"] for c in ENCODE] + [c["name"] for c in LOSS]
    assert len(set(names)) == len(names)
    for want in ("tie_on_border_vertical", "tie_on_border_horizontal", "tie_on_border_corner", "all_iou_zero", "zero_area", "inverted", "image_edges",
                 "overwrite", "ign_thresh_zero", "ign_thresh_one", "ign_thresh_equal", "counts", "no_boxes", "layers_1", "layers_3", "layers_4", "many_images",
                 "clip_hi", "clip_lo", "clip_hi_plain", "clip_lo_plain", "saturated_obj_ale_c2", "saturated_obj_std_c2", "saturated_obj_std_c80",
                 "class_spread_std_c2", "class_spread_std_c80", "wrap", "one_cell_1x1", "one_cell_1x22", "layout") + \
            tuple("class_spread_ale_c%d" % c for c in (1, 2, 3, 80, 128)):
        assert want in names, want
    for c in ENCODE + LOSS:
        for a in ([c["boxes"]] if "boxes" in c else [c["raw"], c["gt"]["loc"]]):
            assert np.isfinite(a).all(), c["name"]


@pytest.mark.parametrize("case", ENCODE, ids=_name)
def test_encode_case_is_what_it_claims(case, oracle_encoded):
    """The predicate that defines the case holds on the float32 oracle's output; ign >= obj always (tfdata.py:154)."""
    enc = oracle_encoded[case["name"]]
    case["check"](case, enc)
    for img in enc:
        assert all((e["ign"] >= e["obj"]).all() and np.isfinite(e["loc"]).all() for e in img)


@pytest.mark.parametrize("case", [c for c in ENCODE if c["name"] not in ("many_images",)], ids=_name)
def test_oracle_encode_equals_the_reference(case, oracle_encoded):
    g = golden("loss_edges.npz")
    assert str(g["enc/%s/inputs" % case["name"]]) == E.input_hash(case), "the case builder no longer makes the inputs of the fixture"
    for i, img in enumerate(oracle_encoded[case["name"]]):
        for k, e in enumerate(img):
            key = "enc/%s/%d/%d/" % (case["name"], i, k)
            for n in ("obj", "cls", "ign"):
                assert np.array_equal(e[n], g[key + n].astype(e[n].dtype)), "%s image %d layer %d %s" % (case["name"], i, k, n)
            assert_close(e["loc"], g[key + "loc"], key + "loc", rtol=1e-6, atol=1e-6)


@pytest.mark.parametrize("case", LOSS, ids=_name)
def test_float32_oracle_reaches_the_bounds(case):
    """A correct float32 implementation (numpy, op for op) is within the bounds the device is held to, and finite."""
    ref = E.reference_loss(case)
    f32 = E.reference_loss(case, np.float32)
    assert all(np.isfinite(ref[k]) and np.isfinite(f32[k]) for k in ("loc", "obj", "cls")) and np.isfinite(ref["grad"]).all() and np.isfinite(f32["grad"]).all()
    d = E.distances([f32[k] for k in ("loc", "obj", "cls")], f32["grad"], ref)
    print(case["name"], "float32 oracle vs float64, fractions of the bound:", {k: float("%.3g" % v) for k, v in d.items()})
    assert max(d.values()) <= 1.0, d
    if case["C"] == 1:
        assert ref["cls"] == 0 and f32["cls"] == 0
        c0 = 10 if case["aleatoric"] else 5
        assert (f32["grad"].reshape(case["raw"].shape[:3] + (3, -1))[..., c0] == 0).all()
    if not case["aleatoric_loss"] and case["aleatoric"]:
        r = case["raw"].reshape(case["raw"].shape[:3] + (3, -1))
        plain = np.sum((case["gt"]["loc"].astype(np.float64) - r[..., 0:4]) ** 2 * case["gt"]["obj"][..., None]) / (2.0 * r.shape[0])
        assert abs(ref["loc"] - plain) <= 1e-12 * plain, "aleatoric_loss = False: the plain squared error"
        assert (ref["grad"].reshape(r.shape)[..., 4:8] == 0).all()


@pytest.mark.parametrize("case", [c for c in LOSS if c["name"] != "wrap"], ids=_name)
def test_oracle_loss_equals_the_reference(case):
    """float64 against float64 at 1e-12 of A (two summation orders of the same terms); float32 against float32 at 2e-6 of max(1, A):
    the bound of tests/test_loss.py, on the scale at which the loc terms cancel."""
    g = golden("loss_edges.npz")
    assert str(g["loss/%s/inputs" % case["name"]]) == E.input_hash(case), "the case builder no longer makes the inputs of the fixture"
    ref = E.reference_loss(case, want_grad=False)
    f32 = E.reference_loss(case, np.float32, want_grad=False)
    for i, k in enumerate(("loc", "obj", "cls")):
        A = max(1.0, float(ref["abs"][k]))
        assert abs(ref[k] - g["loss/%s/f64" % case["name"]][i]) <= 1e-12 * A, (case["name"], k)
        assert abs(float(f32[k]) - g["loss/%s/f32" % case["name"]][i]) <= 2e-6 * A, (case["name"], k)


def _planted_elements(case):
    """(prior box, element of its block, which sum) for the elements the case plants; the clip cases leave out +-40 itself, where the
    clipped log variance has a kink."""
    blk = E.block(case["C"], case["aleatoric"])
    o_obj, c0 = (8, 10) if case["aleatoric"] else (4, 5)
    r = case["raw"].reshape(case["raw"].shape[:3] + (3, blk))
    for p in case["planted"]:
        for e in range(blk):
            if case["aleatoric"] and (e == 9 or e >= c0 + case["C"]):
                continue                                              # the std-dev logits: not in the loss
            if 4 <= e < 8 and case["aleatoric"] and abs(float(r[p][e])) == 40.0:
                continue
            yield p, e, ("loc" if e < (8 if case["aleatoric"] else 4) else "obj" if e == o_obj else "cls")


@pytest.mark.parametrize("case", DERIV, ids=_name)
def test_oracle_gradient_is_the_derivative_at_the_planted_values(case):
    """Central differences in float64, prior box by prior box: the sum an element belongs to, with every OTHER prior box masked out
    (obj = ign = 0) so that a term of 1e17 next door does not drown the quotient; the step 1e-6 keeps x +- step on the same side
    of the clip (39.999 is 1e-3 inside, nextafter(40) 3.8e-6 outside) and grows to 1e-6 * |x| beyond 100, above float64's resolution at
    x = 1e4.  Outside the clip the quotient is exactly 0."""
    from oracle import train_ref
    C, al, all_ = case["C"], case["aleatoric"], case["aleatoric_loss"]
    ana = E.reference_loss(case)["grad"].reshape(case["raw"].shape[:3] + (3, -1))
    raw = case["raw"].astype(np.float64)
    r = raw.reshape(ana.shape)
    worst, n_out = 0.0, 0
    for p, e, which in _planted_elements(case):
        gt = dict(case["gt"], obj=np.zeros_like(case["gt"]["obj"]), ign=np.zeros_like(case["gt"]["ign"]))
        gt["obj"][p], gt["ign"][p] = case["gt"]["obj"][p], case["gt"]["ign"][p]
        v = r[p][e]
        step = 1e-6 * max(1.0, abs(v) / 100.0)
        with np.errstate(over="ignore"):
            r[p][e] = v + step; up = train_ref.loss(raw, gt, C, al, all_)[which]
            r[p][e] = v - step; dn = train_ref.loss(raw, gt, C, al, all_)[which]
        r[p][e] = v
        num = (up - dn) / (2 * step)
        if which == "loc" and 4 <= e < 8 and abs(v) > 40:
            assert num == 0 and ana[p][e] == 0, "outside the clip: no gradient, exactly"
            n_out += 1
        worst = max(worst, abs(ana[p][e] - num) / max(1.0, abs(num)))
        assert abs(ana[p][e] - num) <= 1e-6 * max(1.0, abs(num)), (case["name"], p, e, v, ana[p][e], num)
    assert worst > 0 or case["C"] == 1
    if case["name"].startswith("clip"):
        assert n_out >= 3 * 4 * 4, "nextafter(+-40), +-100 and +-1e4 all met"
