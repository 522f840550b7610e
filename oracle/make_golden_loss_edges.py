"""Oracle (test infrastructure): generate tests/golden/loss_edges.npz by running the reference's OWN `tfdata.encode_boxes`
(lib_yolo/tfdata.py:77-171) and `layers.loss_tf` (lib_yolo/layers.py:126-188), UNMODIFIED under oracle/tf1_shim.py, on the edge
cases of tests/_loss_edges.py (TensorFlow primitives restated from their documented semantics: "parity unpinned" at that boundary,
like oracle/make_golden_loss.py, whose helpers this script uses).

    python -m oracle.make_golden_loss_edges        # from the repo root; needs the reference tree

The fixture holds OUTPUTS only -- per encode case and image the encoded ground truth of every detection layer in float32, per loss
case the three loss terms in float32 and float64 -- and, per case, the SHA-256 of the inputs they were computed from: the tests
rebuild the inputs from tests/_loss_edges.py and compare the hash.  `many_images` (300 images) and `wrap` (3.7 M raw values) are
left out: what they add is the launch geometry, which the reference does not have.  Data only, compressed.
"""
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(REPO, "tests", "golden", "loss_edges.npz")
for p in (os.path.join(REPO, "tests"), REPO):
    if p not in sys.path:
        sys.path.insert(0, p)

from oracle import tf1_shim as shim                  # noqa: E402
from oracle import make_golden as mg                 # noqa: E402
from oracle import make_golden_loss as mgl           # noqa: E402

NOT_IN_FIXTURE = ("many_images", "wrap")


def run_reference_encode_layers(rdata, rtfdata, layers, bboxes, labels, ign_thresh, dtype):
    """make_golden_loss.run_reference_encode for any list of detection layers (h, w, [(prior_h, prior_w)] * 3) and any ign_thresh."""
    shim.install(dtype=dtype)
    infos = [rdata.DetLayerInfo(h=h, w=w, priors=[rdata.Prior(h=p[0], w=p[1]) for p in priors]) for h, w, priors in layers]
    enc = rtfdata.encode_boxes(shim.Tensor(torch.as_tensor(bboxes).to(dtype)), shim.Tensor(torch.as_tensor(labels)), infos, ign_thresh=ign_thresh)
    return [{k: v.numpy() for k, v in e.items()} for e in enc]


def main():
    import _loss_edges as E
    ryolo, rdata, rtfdata, rlayers = mgl.import_training_side()
    out = {}
    for case in E.encode_cases():
        if case["name"] in NOT_IN_FIXTURE:
            continue
        out["enc/%s/inputs" % case["name"]] = np.asarray(E.input_hash(case))
        for i in range(case["boxes"].shape[0]):
            bb, lab = E.image_boxes(case, i)
            enc = run_reference_encode_layers(rdata, rtfdata, case["layers"], bb, lab, case["ign_thresh"], torch.float32)
            for k, e in enumerate(enc):
                out["enc/%s/%d/%d/loc" % (case["name"], i, k)] = e["loc"].astype(np.float32)
                for name in ("obj", "ign"):
                    assert np.isin(e[name], (0, 1)).all()
                    out["enc/%s/%d/%d/%s" % (case["name"], i, k, name)] = e[name].astype(np.uint8)      # masks: 0 / 1
                out["enc/%s/%d/%d/cls" % (case["name"], i, k)] = e["cls"].astype(np.int32)
    for case in E.loss_cases(big=False):
        out["loss/%s/inputs" % case["name"]] = np.asarray(E.input_hash(case))
        for dt, key in ((torch.float32, "f32"), (torch.float64, "f64")):
            out["loss/%s/%s" % (case["name"], key)] = mgl.run_reference_loss(rlayers, case["raw"], case["gt"], case["C"], case["aleatoric"],
                                                                             case["aleatoric_loss"], dt)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes;", len(out), "arrays")
    mg.restore_environment()


if __name__ == "__main__":
    main()
