"""The CPU restatement against the REFERENCE'S OWN graph code: what `lib_yolo/{yolov3,model,layers}.py` and the `inference_*`
helpers computed, executed unmodified under oracle/tf1_shim.py, on weights, images, image size, T and dropout seed that are
NOT the ones the other fixtures were generated with (those pin one configuration; this keeps the restatement from being fitted
to it).  The reference's outputs are stored in tests/golden/ref_cross.npz (oracle/make_golden_cross.py regenerates them where
the reference tree is at hand); the restatement runs live here."""
import numpy as np
import pytest
import torch

from conftest import assert_close, golden
from oracle import make_golden_cross as mgc

VARIANTS = mgc.VARIANTS
H, W, T, SEED_DROP = mgc.H, mgc.W, mgc.T, mgc.SEED_DROP


@pytest.fixture(scope="module")
def ref():
    return golden("ref_cross.npz")


def _params(ref, variant):
    return mgc.params(variant, {k[3:]: ref[k] for k in ref.files if k.startswith("bn/")})


@pytest.mark.parametrize("variant", VARIANTS)
def test_restatement_equals_reference_graph_code(variant, ref):
    from oracle import cpu_ref
    params = _params(ref, variant)
    imgs = mgc.images(variant)
    # in float64 on both sides: the float32 results of the host's convolutions depend on its thread count
    with torch.no_grad():
        boxes, f = cpu_ref.detect_boxes(cpu_ref.to_torch_params(params, torch.float64), imgs, variant, T=T, seed=SEED_DROP, dtype=torch.float64)
    for k in range(3):
        assert_close(f["raw"][k].numpy(), ref["%s/raw64_%d" % (variant, k)], "%s raw detection output %d" % (variant, k), rtol=1e-5, atol=1e-5)
    assert_close(boxes.numpy(), ref["%s/bbox64" % variant], "%s pre-NMS rows" % variant, rtol=1e-5, atol=1e-5)
    rb = ref["%s/bbox" % variant]
    # NMS of the reference's rows: the restated tail on the same rows keeps the same boxes
    mine = cpu_ref.nms_batch(torch.from_numpy(rb), variant)
    for b in range(rb.shape[0]):
        assert np.array_equal(mine[b][0], ref["%s/nms_rows_%d" % (variant, b)]), "%s image %d: NMS rows differ" % (variant, b)
    # structure: variables in creation order, layer count, row layout
    assert ref["%s/var_names" % variant].tolist() == list(cpu_ref.variable_shapes(variant, 2))
    assert tuple(ref["%s/row_layout" % variant].tolist()) == cpu_ref.row_layout(variant, 2)[1:]


def test_injected_masks_mean_the_same_in_the_reference_graph_and_the_restatement(ref):
    """byolo_forward's d_mask_bits hands the product one keep-bit per element of every dropout input, in the order the
    reference CALLS tf.layers.dropout (lib_yolo/layers.py:521-524; yolov3.py:544-548, :575-579, :606-610).  The same
    numpy-drawn arrays given to the reference's own graph code (under the shim) and to the CPU restatement must give
    the same rows: that pins call order and element order of the injection, independently of oracle/rng.py."""
    from oracle import cpu_ref
    from byolo import synth
    variant = "bayesian_yolov3_aleatoric"
    params = _params(ref, variant)
    imgs = synth.synthetic_images(1, H, W, seed=mgc.MASK_IMG_SEED)
    # shapes of the 15 dropout inputs: from a run of the reference itself
    shapes = [tuple(s) for s in ref["masks/shapes"].tolist()]
    assert len(shapes) == 15
    g = np.random.default_rng(mgc.MASK_SEED)
    masks = [g.random(s) < 0.9 for s in shapes]
    tp = cpu_ref.to_torch_params(params, torch.float64)
    with torch.no_grad():
        boxes, f = cpu_ref.detect_boxes(tp, imgs, variant, T=T, seed=555, masks=masks, dtype=torch.float64)
    for k in range(3):
        assert_close(f["raw"][k].numpy(), ref["masks/raw64_%d" % k], "raw detection output %d under injected masks" % k, rtol=1e-5, atol=1e-5)
    assert_close(boxes.numpy(), ref["masks/bbox64"], "pre-NMS rows under injected masks", rtol=1e-5, atol=1e-5)
    # and the masks matter: another draw gives other rows
    other = [g.random(s) < 0.9 for s in shapes]
    with torch.no_grad():
        b2, _ = cpu_ref.detect_boxes(tp, imgs, variant, T=T, seed=555, masks=other, dtype=torch.float64)
    assert np.abs(b2.numpy() - boxes.numpy()).max() > 1e-3


def test_ground_truth_encoding_and_loss_restatement_equal_the_reference_functions(ref):
    """Row f4: oracle/train_ref.py against the reference's `tfdata.encode_boxes` / `layers.loss_tf`, on another image size,
    another prior table, other boxes and raw tensors than the fixture tests/golden/loss_gt.npz."""
    from oracle import make_golden_loss as mgl, train_ref
    table = golden("priors.json")["CITY_PERSONS_9_PRIORS"]
    priors = {s: [tuple(p) for p in table[str(s)]] for s in (32, 16, 8)}
    bb, lab, layers, raws = mgc.loss_inputs(priors)
    enc = train_ref.encode_boxes(bb, lab, layers, mgl.IGN)
    for k in range(3):
        for n in ("obj", "cls", "ign"):
            assert np.array_equal(enc[k][n], ref["encode/%d_%s" % (k, n)]), (k, n)
        assert_close(enc[k]["loc"], ref["encode/%d_loc" % k], "loc %d" % k, rtol=1e-6, atol=1e-6)
    assert sum(int(e["obj"].sum()) for e in enc) >= 9
    for c, (aleatoric, aleatoric_loss) in enumerate(mgc.LOSS_CASES):
        for k in range(3):
            gt = {n: np.stack([enc[k][n]] * 3) for n in ("loc", "obj", "cls", "ign")}
            l = train_ref.loss(raws[c, k], gt, 2, aleatoric, aleatoric_loss)
            assert_close(np.asarray([l["loc"], l["obj"], l["cls"]]), ref["loss/%d_%d" % (c, k)], "loss layer %d" % k, rtol=1e-12, atol=1e-12)
