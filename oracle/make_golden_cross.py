"""Oracle (test infrastructure): generate tests/golden/ref_cross.npz by IMPORTING THE REFERENCE and running its own graph code
(`lib_yolo/{yolov3,model,layers}.py`, the `inference_*` helpers) and its ground-truth encoding and loss (`lib_yolo/tfdata.py`
`encode_boxes`, `lib_yolo/layers.py` `loss_tf`) UNMODIFIED under oracle/tf1_shim.py, on weights, images, image size, T and
dropout seed that are NOT the ones the other fixtures were generated with.  tests/test_oracle_vs_reference.py holds the CPU
restatement to these outputs (the other fixtures pin one configuration; this keeps the restatement from being fitted to it).

    python -m oracle.make_golden_cross        # from the repo root; needs the reference tree (make_golden.REF)

Data only: the reference's outputs, the BN statistics of the weights and the shapes of the reference's dropout inputs; the
inputs themselves are regenerated from the seeds below (byolo/synth.py, numpy's default_rng).
"""
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(REPO, "tests", "golden", "ref_cross.npz")
sys.path.insert(0, REPO)

from oracle import cpu_ref                           # noqa: E402
from oracle import make_golden as mg                 # noqa: E402

VARIANTS = ("yolov3", "yolov3_aleatoric", "bayesian_yolov3_aleatoric")
H, W, T, SEED_W, SEED_DROP = 32, 64, 2, 21, 77
MASK_SEED, MASK_IMG_SEED = 2024, 33
LOSS_SEED, LOSS_HW, LOSS_BOXES = 99, (96, 160), 9
LOSS_CASES = ((False, False), (True, False), (True, True))          # (aleatoric, aleatoric_loss)


def calibrated_stats():
    """BN statistics calibrated once with the restatement (oracle/make_golden.py calibrated_params does the same for the other
    fixtures); stored in the fixture, so the test rebuilds exactly these weights."""
    shapes = cpu_ref.variable_shapes("yolov3_aleatoric", 2)
    p = cpu_ref.to_torch_params(mg.synth.base_params(shapes, "yolov3_aleatoric", 2, seed=SEED_W))
    with torch.no_grad():
        cpu_ref.forward(p, mg.synth.synthetic_images(32, H, W, seed=5), "yolov3_aleatoric", calibrate=True)
    return {k: v.numpy().astype(np.float32) for k, v in p.items() if k.endswith("moving_mean") or k.endswith("moving_variance")}


def params(variant, stats):
    out = mg.synth.base_params(cpu_ref.variable_shapes(variant, 2), variant, 2, seed=SEED_W)
    for k, v in stats.items():
        out[k] = np.asarray(v, np.float32)
    return out


def images(variant):
    return mg.synth.synthetic_images(1 if variant.startswith("bayes") else 2, H, W, seed=31)   # the reference asserts batch 1 in epistemic mode


def loss_inputs(priors):
    """Boxes, labels, detection layers and the raw tensors of the loss cases, drawn from one seeded stream in a fixed order."""
    from oracle import make_golden_loss as mgl
    rng = np.random.default_rng(LOSS_SEED)
    hw = LOSS_HW
    flat = [(h, w) for s in (32, 16, 8) for h, w in priors[s]]
    bb, lab = mgl.boxes_for(rng, LOSS_BOXES, hw[0] // 16, hw[1] // 16, flat)
    layers = [(hw[0] // s, hw[1] // s, [tuple(p) for p in priors[s]]) for s in (32, 16, 8)]
    raws = {}
    for c, (aleatoric, _) in enumerate(LOSS_CASES):
        for k, (lh, lw, _) in enumerate(layers):
            raws[c, k] = (rng.standard_normal((3, lh, lw, 3 * (14 if aleatoric else 7))) * 2.0).astype(np.float32)
    return bb, lab, layers, raws


def main():
    mg.restore_environment()
    saved = (mg.H, mg.W)
    mg.H, mg.W = H, W
    try:
        out = {}
        stats = calibrated_stats()
        for k, v in stats.items():
            out["bn/" + k] = v
        # 1. the three variants' forwards
        # (raw outputs and rows in float64, where the summation order of the host's convolutions does not show; the float32 rows
        # and what the reference's NMS keeps of them, for the tail)
        for variant in VARIANTS:
            ref = mg.run_reference(variant, params(variant, stats), images(variant), torch.float32, seed=SEED_DROP, T=T)
            ref64 = mg.run_reference(variant, params(variant, stats), images(variant), torch.float64, seed=SEED_DROP, T=T)
            for k in range(3):
                out["%s/raw64_%d" % (variant, k)] = ref64["raw"][k].astype(np.float64)
            out["%s/bbox64" % variant] = (ref64["bbox"] if ref64["bbox"].ndim == 3 else ref64["bbox"][None]).astype(np.float64)
            out["%s/bbox" % variant] = (ref["bbox"] if ref["bbox"].ndim == 3 else ref["bbox"][None]).astype(np.float32)
            for b, rows in enumerate(ref["nms_rows"]):
                out["%s/nms_rows_%d" % (variant, b)] = rows.astype(np.float32)
            out["%s/var_names" % variant] = np.asarray(ref["var_names"])
            out["%s/row_layout" % variant] = np.asarray([ref["obj_idx"], ref["cls_start_idx"]], np.int32)
        # 2. injected dropout masks: shapes of the 15 dropout inputs from a probe run, then the reference on seeded masks
        variant = "bayesian_yolov3_aleatoric"
        p = params(variant, stats)
        imgs = mg.synth.synthetic_images(1, H, W, seed=MASK_IMG_SEED)
        probe = mg.run_reference(variant, p, imgs, torch.float32, seed=1, T=T)
        shapes = [tuple(s) for _, s in probe["dropout_calls"]]
        g = np.random.default_rng(MASK_SEED)
        masks = [g.random(s) < 0.9 for s in shapes]
        ref = mg.run_reference(variant, p, imgs, torch.float64, seed=999, T=T, masks=masks)
        out["masks/shapes"] = np.asarray([list(s) for s in shapes], np.int64)
        for k in range(3):
            out["masks/raw64_%d" % k] = ref["raw"][k].astype(np.float64)
        out["masks/bbox64"] = ref["bbox"][None].astype(np.float64)
        # 3. ground-truth encoding and the loss terms
        from oracle import make_golden_loss as mgl
        ryolo, rdata, rtfdata, rlayers = mgl.import_training_side()
        priors = {s: [(q.h, q.w) for q in ryolo.CITY_PERSONS_9_PRIORS[s]] for s in (32, 16, 8)}
        bb, lab, layers, raws = loss_inputs(priors)
        enc = mgl.run_reference_encode(rdata, rtfdata, LOSS_HW, ryolo.CITY_PERSONS_9_PRIORS, bb, lab, torch.float32)
        for k in range(3):
            for n in ("obj", "cls", "ign", "loc"):
                out["encode/%d_%s" % (k, n)] = enc[k][n]
        # the loss terms on the restatement's encoding, as the test evaluates its own loss (the encodings agree: the test checks)
        from oracle import train_ref
        mine = train_ref.encode_boxes(bb, lab, layers, mgl.IGN)
        for c, (aleatoric, aleatoric_loss) in enumerate(LOSS_CASES):
            for k in range(3):
                gt = {n: np.stack([mine[k][n]] * 3) for n in ("loc", "obj", "cls", "ign")}
                out["loss/%d_%d" % (c, k)] = mgl.run_reference_loss(rlayers, raws[c, k], gt, 2, aleatoric, aleatoric_loss, torch.float64)
        np.savez_compressed(OUT, **out)
        print(OUT, os.path.getsize(OUT), "bytes")
    finally:
        mg.H, mg.W = saved
        mg.restore_environment()


if __name__ == "__main__":
    main()
