#!/usr/bin/env python
"""box_vote_time.py -- device time of the tail (what profiling stage 3 of a forward covers: the launches of byolo_sort_nms and,
with voting on, of byolo_box_vote right behind them) with variance voting off and on, on the Bayesian rows of
tests/_box_vote_ref.py:

    clustered   24 clusters of large boxes: few kept rows, thousands of voters each (the float64 path at its busiest)
    spread      4000 clusters of small boxes: max_out kept rows, a handful of voters each (the float32 IoU test dominates)

at N = 22 743 x B = 8 (608 x 608) and N = 120 960 x B = 11 (1920 x 1024), class-agnostic and per-class (two classes) NMS.

    python tools/box_vote_time.py --out out/box_vote.json --md profiles/box_vote.md
    python tools/box_vote_time.py --pkg <another checkout>/bayesian-yolov3_amd --no-vote --label parent    # a tree without the stage

Per case: warm-up calls, then `--repeats` windows of `--calls` back-to-back calls between two device events; the figure is the
median window / calls with the fastest and slowest window beside it.  `off` is sort_nms alone, `on` sort_nms + box_vote; what
voting adds is their difference.  --step-ms: the time of a whole forward step at the first size (bench.py's ms_per_step), to
print the addition as a share of it."""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = ((22743, 8), (120960, 11))
ROWS = {"clustered": dict(n_clusters=24, jitter=0.01, half=0.06), "spread": dict(n_clusters=4000, jitter=0.001, half=0.008)}
VARIANT, C = "bayesian_yolov3_aleatoric", 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pkg", default=os.path.join(REPO, "bayesian-yolov3_amd"), help="the package directory to import byolo from")
    ap.add_argument("--modes", default="0,2")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-vote", action="store_true", help="time sort_nms alone (a tree that has no voting stage)")
    ap.add_argument("--step-ms", type=float, default=0.0)
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default="")
    ap.add_argument("--md", default="")
    a = ap.parse_args()
    sys.path.insert(0, REPO)
    sys.path.insert(0, os.path.join(REPO, "tests"))
    sys.path.insert(0, a.pkg)
    import torch
    import _box_vote_ref as bv
    from byolo import Engine
    assert torch.cuda.is_available(), "a timing needs the GPU"
    L = bv.layout(VARIANT, C)

    def timed(run):
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
        return dict(ms_median=round(ms[len(ms) // 2], 4), ms_min=round(ms[0], 4), ms_max=round(ms[-1], 4)), res

    results = []
    for N, B in SIZES:
        for kind, kw in ROWS.items():
            # one image's rows, repeated over the batch with rolled order: generating 11 x 120 960 rows takes longer than timing them
            one = bv.random_rows(np.random.default_rng(N % 1000), 1, N, VARIANT, C, **kw)[0]
            rows = torch.from_numpy(np.stack([np.roll(one, 97 * b, axis=0) for b in range(B)])).cuda()
            for mode in (int(m) for m in a.modes.split(",")):
                eng = Engine((64, 64, 3), C, nms_mode=mode)
                nms = lambda: eng.sort_nms(rows, obj_idx=L["obj_idx"], cls_start_idx=L["cls_start"])
                off, res = timed(nms)
                r = dict(label=a.label, rows=kind, mode=mode, N=N, B=B, off=off, kept=res["count"][:, 0].cpu().tolist()[:2])
                if not a.no_vote:
                    def both():
                        n = nms()
                        return eng.box_vote(rows, n, L["obj_idx"], L["cls_start"], geom=bv.GEOM, var="total")
                    on, voted = timed(both)
                    vn = voted["vote_n"][0, :r["kept"][0]].cpu().numpy()
                    r.update(on=on, adds_ms=round(on["ms_median"] - off["ms_median"], 4), voters_median=int(np.median(vn)) if len(vn) else 0,
                             voters_max=int(vn.max()) if len(vn) else 0)
                results.append(r)
                print(json.dumps(r), flush=True)
                eng.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)
    if a.md:
        lines = ["| rows | NMS mode | B x N | kept (image 0) | voters median / max | tail, voting off, ms (min .. max) | tail, voting on, ms (min .. max) | voting adds, ms | of the off tail |" +
                 (" of the step |" if a.step_ms else ""), "|---|---|---|---|---|---|---|---|---|" + ("---|" if a.step_ms else "")]
        for r in results:
            if "on" not in r:
                lines.append("| %s | %d | %d x %d | %d | - | %.3f (%.3f .. %.3f) | - | - | - |" % (
                    r["rows"], r["mode"], r["B"], r["N"], r["kept"][0], r["off"]["ms_median"], r["off"]["ms_min"], r["off"]["ms_max"]))
                continue
            line = "| %s | %d | %d x %d | %d | %d / %d | %.3f (%.3f .. %.3f) | %.3f (%.3f .. %.3f) | %.3f | %.0f %% |" % (
                r["rows"], r["mode"], r["B"], r["N"], r["kept"][0], r["voters_median"], r["voters_max"], r["off"]["ms_median"], r["off"]["ms_min"],
                r["off"]["ms_max"], r["on"]["ms_median"], r["on"]["ms_min"], r["on"]["ms_max"], r["adds_ms"], 100 * r["adds_ms"] / r["off"]["ms_median"])
            if a.step_ms:
                line += (" %.2f %% |" % (100 * r["adds_ms"] / a.step_ms)) if r["N"] == SIZES[0][0] else " - |"
            lines.append(line)
        os.makedirs(os.path.dirname(os.path.abspath(a.md)), exist_ok=True)
        with open(a.md, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
