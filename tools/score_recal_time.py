#!/usr/bin/env python
"""score_recal_time.py -- what score recalibration costs on the device (profiles/score_recal.md):

    apply     the stand-alone stage (Engine.score_recal, out of place) on 1, 8 and 11 images x cap kept rows of Bayesian rows with 2
              classes (cap = 1000 x 2 under the per-class NMS, every row kept), the default 7 features, by 'all' and by 'class'
    fit       byolo.score_recal.fit_arrays at 10^4, 10^5 and 10^6 records, K = 7: ONE group (by 'all': one workgroup does it all)
              and 2 classes + 'all' (by 'class'), host clock around the call (it ends in the copy of the result to the host)

    python tools/score_recal_time.py --out out/score_recal.json

Per apply case: warm-up calls, then `--repeats` windows of `--calls` back-to-back calls between two device events; the figure is
the median window / calls with the fastest and slowest window beside it."""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--records", type=int, nargs="*", default=[10000, 100000, 1000000])
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(REPO, "bayesian-yolov3_amd"))
    import torch
    from byolo import Engine, score_recal as sr
    assert torch.cuda.is_available(), "a timing needs the GPU"
    rng = np.random.default_rng(0)
    variant, C = "bayesian_yolov3_aleatoric", 2

    def window(run):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.calls):
            run()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.calls

    def stats(ms):
        ms = sorted(ms)
        return dict(ms_median=round(ms[len(ms) // 2], 4), ms_min=round(ms[0], 4), ms_max=round(ms[-1], 4))

    def cal(by):
        c = sr.ScoreCalibration(variant, C, None, by)
        c.w = [[float(rng.normal(0, 0.5)), float(rng.uniform(0.5, 1.5))] + [float(v) for v in rng.normal(0, 0.2, c.K - 2)] for _ in range(c.n_groups)]
        return c

    results = {"apply": {}, "fit": {}}
    eng = Engine((64, 64, 3), C)
    cap, D = 2000, 21 + C
    for B in (1, 8, 11):
        rows = torch.from_numpy(rng.uniform(0.01, 1.0, (B, cap, D)).astype(np.float32)).cuda()
        count = torch.full((B, 2), cap, dtype=torch.int32, device="cuda")
        for by in ("all", "class"):
            c = cal(by)
            run = lambda: eng.score_recal(rows, count, c)
            for _ in range(a.warmup):
                run()
            results["apply"]["B%d_%s" % (B, by)] = dict(stats([window(run) for _ in range(a.repeats)]), rows=B * cap)
    print(json.dumps(results["apply"]), flush=True)
    eng.close()

    K = 7
    coef = np.array([0.3, 1.5, -0.2, -0.4, 0.3, -1.0, 0.5])
    for n in a.records:
        x = np.concatenate([np.ones((n, 1)), rng.normal(0.0, 2.0, (n, 1)), rng.normal(0.0, 1.0, (n, K - 2))], axis=1)
        y = (rng.uniform(0, 1, n) < 1.0 / (1.0 + np.exp(-(x @ coef)))).astype(np.float64)
        cls = rng.integers(0, C, n)
        xd, yd, cd = (torch.from_numpy(v).cuda() for v in (x, y, cls))
        for by in ("all", "class"):
            if by == "all":
                args = (xd, yd, torch.zeros_like(cd), 1)
            else:
                args = (torch.cat([xd, xd]), torch.cat([yd, yd]), torch.cat([cd, torch.full_like(cd, C)]), C + 1)
            seg = sr.fit_arrays(*args, 1.0, 200)
            ms = []
            for _ in range(max(1, a.repeats // 2)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                seg = sr.fit_arrays(*args, 1.0, 200)
                ms.append((time.perf_counter() - t0) * 1e3)
            results["fit"]["n%d_%s" % (n, by)] = dict(stats(ms), iterations_max=int(seg["iterations"].max()), converged=bool(seg["converged"].all()))
            print(json.dumps({"n%d_%s" % (n, by): results["fit"]["n%d_%s" % (n, by)]}), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
