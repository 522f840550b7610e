#!/usr/bin/env python
"""nms_per_class_time.py -- device time of the NMS tail (Engine.sort_nms: score sort + greedy NMS + gather) per mode and
class count, on the random rows of tests/_nms_per_class_ref.py (tied scores and class scores, one class far beyond max_out).

    python tools/nms_per_class_time.py --cases 2:2,2:3,2:7,2:80,0:3 --out out/nms_time.json
    python tools/nms_per_class_time.py --pkg <another checkout>/bayesian-yolov3_amd --cases 1:2 ...    # that checkout's library

A case is mode:C (BYOLO_NMS_* mode, class count).  Each case runs at both sizes (N = 22 743 x B = 8, the 608 x 608 box count;
N = 120 960 x B = 11, 1920 x 1024).  Per case: warm-up calls, then `--repeats` windows of `--calls` back-to-back calls between
two device events; the figure is the median window / calls, with the fastest and slowest window beside it (the spread of the
box).  One JSON line per case on stdout, all of them in --out."""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = ((22743, 8), (120960, 11))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="2:2,2:3,2:7,2:80,0:3")
    ap.add_argument("--pkg", default=os.path.join(REPO, "bayesian-yolov3_amd"), help="the package directory to import byolo from")
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    sys.path.insert(0, REPO)
    sys.path.insert(0, os.path.join(REPO, "tests"))
    sys.path.insert(0, a.pkg)
    import torch
    import _nms_per_class_ref as pcr
    from byolo import Engine
    assert torch.cuda.is_available(), "a timing needs the GPU"
    results = []
    for case in a.cases.split(","):
        mode, C = (int(v) for v in case.split(":"))
        for N, B in SIZES:
            # the same rows for every mode at one (C, size): the seed does not depend on the mode
            rows = torch.from_numpy(pcr.random_rows(np.random.default_rng(1000 + C), B, N, C)).cuda()
            eng = Engine((64, 64, 3), C, nms_mode=mode)
            run = lambda: eng.sort_nms(rows, obj_idx=pcr.OBJ_IDX, cls_start_idx=pcr.CLS_START)
            for _ in range(a.warmup):
                res = run()
            torch.cuda.synchronize()
            ms = []
            for _ in range(a.repeats):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.calls):
                    res = run()
                e1.record()
                torch.cuda.synchronize()
                ms.append(e0.elapsed_time(e1) / a.calls)
            ms.sort()
            r = dict(label=a.label, mode=mode, cls_cnt=C, N=N, B=B, ms_median=round(ms[len(ms) // 2], 4), ms_min=round(ms[0], 4),
                     ms_max=round(ms[-1], 4), kept=res["count"][:, 0].cpu().tolist(), repeats=a.repeats, calls=a.calls)
            results.append(r)
            print(json.dumps(r), flush=True)
            eng.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
