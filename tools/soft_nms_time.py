#!/usr/bin/env python
"""soft_nms_time.py -- device time of the tail (what profiling stage 3 of a forward covers) with the hard NMS (Engine.sort_nms)
against the soft-NMS (Engine.soft_nms) on the same rows, and -- with --step -- the headline forward with the stage off and on.

    python tools/soft_nms_time.py --out out/soft_nms.json [--step]

Rows: 8 images of N = 22 743 (608 x 608) and N = 120 960 (1920 x 1024) rows from tests/_nms_per_class_ref.random_rows, as
  sparse    small boxes all over the image, 2 % of the rows score above min_score (the others are scaled to below 1e-4)
  crowded   the same 2 %, as 40 tight clusters: what a crowd gives a detector
  dense     the 40 clusters with EVERY row a candidate -- at N = 120 960 more than the resident capacity per class: the path that
            keeps the current scores in the workspace
One class (BYOLO_NMS_AGNOSTIC) and two (BYOLO_NMS_TWO_CLASS), both methods, default settings.  Per case: warm-up calls, then
`--repeats` windows of `--calls` back-to-back calls between two device events; the figure is the median window / calls with the
fastest and slowest window beside it.  One JSON line per case on stdout, all of them in --out.

--step: the flagship configuration of bench.py (bayesian_yolov3_aleatoric, 608 x 608, T = 30, 8 images, synthetic weights):
ms per forward over `--steps` back-to-back forwards and the stage-3 time of the profiler, with the soft-NMS off and on."""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (22743, 120960)
B = 8


def make_rows(pcr, kind, N, seed):
    g = np.random.default_rng([77, seed])
    rows = pcr.random_rows(g, B, N, 2, boxes="spread" if kind == "sparse" else "clustered")
    if kind != "dense":
        low = g.random((B, N)) >= 0.02
        rows[..., pcr.OBJ_IDX] = np.where(low, rows[..., pcr.OBJ_IDX] * np.float32(1e-4), np.maximum(rows[..., pcr.OBJ_IDX], np.float32(0.002)))
    return rows


def windows(torch, run, warmup, repeats, calls):
    for _ in range(warmup):
        res = run()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            res = run()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / calls)
    ms.sort()
    return res, dict(ms_median=round(ms[len(ms) // 2], 4), ms_min=round(ms[0], 4), ms_max=round(ms[-1], 4))


def step_leg(torch, steps, warmup):
    from byolo import synth
    from lib_yolo import yolov3, model
    out = []
    for soft in (None, {"method": "gaussian"}, {"method": "linear"}):
        opts = {"nms_mode": 0}
        if soft:
            opts["soft_nms"] = soft
        config = {"full_img_size": [608, 608, 3], "crop": False, "cls_cnt": 2, "priors": yolov3.ECP_9_PRIORS, "aleatoric_loss": False,
                  "inference_mode": True, "T": 30, "implicit_background_class": True, "engine_options": opts}
        m = yolov3.bayesian_yolov3_aleatoric(config).init_model(inputs=model.Placeholder((None, 608, 608, 3)), training=False).get_model()
        eng = m.engine
        eng.set_params(synth.base_params(eng.param_shapes(), "bayesian_yolov3_aleatoric", 2, seed=7))
        eng.finalize()
        eng.calibrate_bn(torch.from_numpy(synth.synthetic_images(2, 608, 608, seed=999)).cuda())
        eng.set_async(True)
        x = torch.from_numpy(synth.synthetic_images(B, 608, 608, seed=1234)).cuda()
        for i in range(warmup):
            res = eng.forward(x, T=30, seed=1000 + i, want_boxes=False, want_nms=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(steps):
            eng.forward(x, T=30, seed=1000 + warmup + i, want_boxes=False, want_nms=True)
        torch.cuda.synchronize()
        ms_step = (time.perf_counter() - t0) * 1e3 / steps
        res = eng.forward(x, T=30, seed=1000, want_boxes=True, want_nms=True)
        eng.set_profiling(1)
        tails = []
        for i in range(5):
            eng.forward(x, T=30, seed=1000 + i, want_boxes=False, want_nms=True)
            torch.cuda.synchronize()
            tails.append(eng.stage_ms()["sort_nms"])
        eng.set_profiling(0)
        above = (res["boxes"][..., m.obj_idx] > 0.001).sum(1).cpu().tolist()
        r = dict(leg="step", soft=soft, ms_per_step=round(ms_step, 3), stage3_ms=round(sorted(tails)[2], 4), kept=res["count"][:, 0].cpu().tolist(),
                 rows_above_min_score=above, steps=steps)
        out.append(r)
        print(json.dumps(r), flush=True)
        eng.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--step", action="store_true", help="also time the flagship forward with the stage off and on")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    for p in (REPO, os.path.join(REPO, "tests"), os.path.join(REPO, "bayesian-yolov3_amd")):
        sys.path.insert(0, p)
    import torch
    import _nms_per_class_ref as pcr
    from byolo import Engine
    assert torch.cuda.is_available(), "a timing needs the GPU"
    results = []
    for N in SIZES:
        for kind in ("sparse", "crowded", "dense"):
            rows_np = make_rows(pcr, kind, N, len(kind))
            rows = torch.from_numpy(rows_np).cuda()
            for mode in (0, 1):
                eng = Engine((64, 64, 3), 2, nms_mode=mode)
                cand = int((rows_np[0, :, pcr.OBJ_IDX] > 0.001).sum())
                res, t = windows(torch, lambda: eng.sort_nms(rows, pcr.OBJ_IDX, pcr.CLS_START), a.warmup, a.repeats, a.calls)
                legs = [("hard", res, t)]
                for method in ("linear", "gaussian"):
                    # a dense image costs tens of milliseconds per call: fewer calls per window there
                    calls = 1 if kind == "dense" else a.calls
                    res, t = windows(torch, lambda: eng.soft_nms(rows, pcr.OBJ_IDX, pcr.CLS_START, method=method), 1 if kind == "dense" else a.warmup,
                                     a.repeats, calls)
                    legs.append((method, res, t))
                for name, res, t in legs:
                    r = dict(leg="stage", rows=kind, N=N, B=B, mode=mode, nms=name, candidates_image0=cand, kept=res["count"][:, 0].cpu().tolist()[:2], **t)
                    results.append(r)
                    print(json.dumps(r), flush=True)
                eng.close()
    if a.step:
        results += step_leg(torch, a.steps, 5)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
