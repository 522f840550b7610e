"""Time byolo.train.HeadTrainer steps at the reference's training workloads (device events after warm-up, feed excluded):

    bayes   768 x 1440 crop, B = 2, bayesian_yolov3_aleatoric, inference_mode=False, aleatoric loss  (uncertainty_training.py)
    yolov3  768 x 1440 crop, B = 8, yolov3                                                           (yolov3_training.py)

and count the heads' forward + backward FLOPs from the layer shapes (per convolution: forward 2 M K N, wgrad 2 M K N, dgrad 2 M K N
where the input carries gradient; M = B H W, K = k k Cin, N = Cout).  Per-kernel times come from a separate
`rocprofv3 --kernel-trace --stats -- python tools/train_step_time.py --steps 3` run.

    python tools/train_step_time.py [--steps 20] [--warmup 3] [--only bayes|yolov3] [--json out.json]
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "bayesian-yolov3_amd"), os.path.join(REPO, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

PEAK_F32 = 157.3e12          # fp32 matrix = fp32 vector peak of the MI355X (MI355X_MICROARCH.md)
WORKLOADS = {"bayes": ("bayesian_yolov3_aleatoric", 768, 1440, 2), "yolov3": ("yolov3", 768, 1440, 8)}


def head_flops(variant, H, W, B, cls_cnt=2):
    from oracle import cpu_ref
    topo = cpu_ref.topology(variant, cls_cnt, False)
    shapes = cpu_ref.variable_shapes(variant, cls_cnt)
    out = {"fwd": 0.0, "wgrad": 0.0, "dgrad": 0.0}
    stride = {"det_net_1": 32, "det_net_2": 16, "det_net_3": 8}
    for i, l in enumerate(topo[75:], 75):
        if l["op"] not in ("conv", "detection"):
            continue
        scope = l["scope"]
        k, _, cin, cout = shapes[scope + "/conv2d/kernel"]
        s = stride[scope.split("/")[0]]
        f = 2.0 * B * (H // s) * (W // s) * k * k * cin * cout
        out["fwd"] += f
        out["wgrad"] += f
        first = scope.endswith("det_net_1/conv")                # reads only the backbone tap: no dgrad
        if not first:
            out["dgrad"] += f
    out["total"] = out["fwd"] + out["wgrad"] + out["dgrad"]
    return out


def run(name, steps, warmup):
    from byolo import synth
    from byolo.train import HeadTrainer
    from conftest import build_model
    variant, H, W, B = WORKLOADS[name]
    kw = {"inference_mode": False} if variant == "bayesian_yolov3_aleatoric" else {}
    _, m = build_model(variant, H, W, aleatoric_loss=variant != "yolov3", **kw)
    m.engine.set_params(synth.base_params(m.engine.param_shapes(), variant, 2, seed=7))
    img = torch.from_numpy(synth.synthetic_images(B, H, W, seed=5)).cuda()
    m.finalize()
    m.engine.calibrate_bn(img)
    rng = np.random.default_rng(0)
    boxes = np.sort(rng.uniform(0, 1, (B, 20, 4)).astype(np.float32), axis=-1)      # (ymin, xmin, ymax, xmax) with ymin < ymax, xmin < xmax
    labels = rng.integers(0, 2, (B, 20)).astype(np.int32)
    tr = HeadTrainer(m, lr=1e-4, seed=1)
    for _ in range(warmup):
        tr.step(img, boxes, labels)
    torch.cuda.synchronize()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for _ in range(steps):
        ev0.record()
        tr.step(img, boxes, labels)                            # (the step reads its losses back: one sync per step)
        ev1.record()
        torch.cuda.synchronize()
        times.append(ev0.elapsed_time(ev1))
    fl = head_flops(variant, H, W, B)
    ms = float(np.median(times))
    tr.close()
    m.engine.close()
    return {"workload": name, "variant": variant, "H": H, "W": W, "B": B, "steps": steps, "ms_per_step_median": ms,
            "ms_per_step_min": float(np.min(times)), "ms_per_step_max": float(np.max(times)),
            "head_gflop": {k: v / 1e9 for k, v in fl.items()},
            "head_gemm_tflops_if_all_step_time": fl["total"] / (ms * 1e-3) / 1e12,
            "share_of_fp32_peak_if_all_step_time": fl["total"] / (ms * 1e-3) / PEAK_F32}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", choices=sorted(WORKLOADS))
    ap.add_argument("--json")
    a = ap.parse_args()
    res = [run(n, a.steps, a.warmup) for n in WORKLOADS if a.only in (None, n)]
    for r in res:
        print(json.dumps(r), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
