"""Time the training feed (lib_yolo.dataset_utils.TrainValDataset + csrc/augment.hip) on one MI355X:

    --kernel   byolo_augment_batch at B = 8 from 1024 x 1920 frames to 768 x 1440: plans drawn by byolo/augment.py (the
               typical mix), and a worst case where every image rescales, blurs with k = 3, shifts hue and adds Gaussian noise
               (device events around N launches; per-kernel times come from a separate
               `rocprofv3 --kernel-trace --stats -- python tools/train_feed_time.py --kernel` run)
    --feed     steps per second of HeadTrainer fed from TFRecord shards (1024 x 1920 PNG frames generated here from a seed,
               cropped to 768 x 1440) against HeadTrainer.step on a resident device batch: yolov3 B = 8 and
               bayesian_yolov3_aleatoric B = 2 (profiles/train_heads_step.md)

    python tools/train_feed_time.py --kernel [--iters 50] [--json out.json]
    python tools/train_feed_time.py --feed [--only yolov3|bayes] [--steps 30] [--warmup 5] [--threads 16 [12 ...]] [--json out.json]
    python tools/train_feed_time.py --kernel --feed --threads 16 8 --rocprof-db DB --profile profiles/train_feed

--rocprof-db: the database of the separate rocprofv3 run (`-o` / `-d`: <dir>/<name>_results.db); its augment launches are split
into the three plan sets in launch order.  --profile PREFIX writes PREFIX.json (everything measured) and PREFIX.md (the tables).
"""
import argparse
import json
import os
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "bayesian-yolov3_amd"), os.path.join(REPO, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

HF, WF, HC, WC = 1024, 1920, 768, 1440
NOTES = "<!-- notes: kept by --profile -->"
WORKLOADS = {"bayes": ("bayesian_yolov3_aleatoric", 2), "yolov3": ("yolov3", 8)}


def kernel(iters, B=8):
    from byolo import augment
    cfg = {"crop": True, "crop_img_size": [HC, WC, 3], "full_img_size": [HF, WF, 3], "seed": 0}
    frames = torch.from_numpy(np.random.default_rng(0).integers(0, 256, (B, HF, WF, 3), dtype=np.uint8)).cuda()
    drawn = augment.empty_plans(B)
    for b in range(B):
        augment.draw(cfg, "train", 0, b, drawn[b])
    worst = augment.empty_plans(B)
    for b in range(B):
        worst[b]["y0"], worst[b]["x0"], worst[b]["ch"], worst[b]["cw"], worst[b]["rescale"] = 0, 0, HF, WF, 1
        worst[b]["blur_k"], worst[b]["color_op"], worst[b]["color_param"] = 3, 3, 0.13
        worst[b]["noise_op"], worst[b]["noise_param"], worst[b]["noise_key"] = 3, 0.03, 1234 + b
    plain = augment.empty_plans(B)
    for b in range(B):
        plain[b]["y0"], plain[b]["x0"], plain[b]["ch"], plain[b]["cw"] = 128, 240, HC, WC
    out = torch.empty((B, HC, WC, 3), dtype=torch.float32, device="cuda")
    res = {}
    for name, plans in (("plain_crop", plain), ("drawn", drawn), ("worst", worst)):
        for _ in range(3):
            augment.augment_batch(frames, plans, (HC, WC), out=out)
        torch.cuda.synchronize()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(iters + 1)]
        ev[0].record()
        for i in range(iters):
            augment.augment_batch(frames, plans, (HC, WC), out=out)
            ev[i + 1].record()
        torch.cuda.synchronize()
        us = [ev[i].elapsed_time(ev[i + 1]) * 1e3 for i in range(iters)]
        read = sum(int(p["ch"]) * int(p["cw"]) * 3 for p in plans)
        res[name] = {"us_median": float(np.median(us)), "us_min": float(np.min(us)), "iters": iters,
                     "plans": [{k: (int(p[k]) if k != "color_param" and k != "noise_param" else float(p[k]))
                                for k in ("ch", "cw", "rescale", "flip", "blur_k", "color_op", "noise_op")} for p in plans],
                     "min_bytes_read": read, "bytes_written": B * HC * WC * 3 * 4}
        print(json.dumps({name: {k: v for k, v in res[name].items() if k != "plans"}}), flush=True)
    return res


def feed(name, steps, warmup, threads, folder):
    from byolo import synth
    from byolo.train import HeadTrainer
    from conftest import build_model
    from lib_yolo import dataset_utils, yolov3
    variant, B = WORKLOADS[name]
    pattern = os.path.join(folder, "synth-train-*-of-*")
    if not os.path.exists(os.path.join(folder, "synth-train-00000-of-00002")):
        t0 = time.time()
        synth.training_shards(folder, 2, 12, HF, WF, seed=7)
        print("shards written in %.1f s" % (time.time() - t0), flush=True)
    kw = {"inference_mode": False} if variant == "bayesian_yolov3_aleatoric" else {}
    _, m = build_model(variant, HC, WC, aleatoric_loss=variant != "yolov3", **kw)
    m.engine.set_params(synth.base_params(m.engine.param_shapes(), variant, 2, seed=7))
    m.finalize()
    m.engine.calibrate_bn(torch.from_numpy(synth.synthetic_images(B, HC, WC, seed=5)).cuda())
    tr = HeadTrainer(m, lr=1e-5, seed=1)
    cfg = {"crop": True, "crop_img_size": [HC, WC, 3], "full_img_size": [HF, WF, 3], "batch_size": B, "cpu_thread_cnt": threads,
           "implicit_background_class": True, "seed": 0,
           "train": {"file_pattern": pattern, "num_shards": 2, "shuffle_buffer_size": 2000, "cache": True},
           "val": {"file_pattern": pattern, "num_shards": 2, "shuffle_buffer_size": 10, "cache": True}}
    ds = dataset_utils.TrainValDataset(None, cfg)
    try:
        for _ in range(max(warmup, 24 // B + 1)):        # warm-up, and one epoch so that every payload is cached
            b = next(ds.train)
            tr.step(b["img"], b["boxes"], b["labels"], b["counts"])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        in_next = 0.0
        ds.train.host_seconds = {k: 0.0 for k in ds.train.host_seconds}
        for s in range(steps):
            t1 = time.perf_counter()
            b = next(ds.train)
            in_next += time.perf_counter() - t1
            tr.step(b["img"], b["boxes"], b["labels"], b["counts"], seed=s)
        torch.cuda.synchronize()
        fed = (time.perf_counter() - t0) / steps
        host = dict(ds.train.host_seconds)
        img = b["img"].clone()
        boxes, labels, counts = b["boxes"], b["labels"], b["counts"]
        t0 = time.perf_counter()
        for s in range(steps):
            tr.step(img, boxes, labels, counts, seed=s)
        torch.cuda.synchronize()
        resident = (time.perf_counter() - t0) / steps
    finally:
        ds.close()
        tr.close()
        m.engine.close()
    r = {"workload": name, "variant": variant, "B": B, "frames": [HF, WF], "crop": [HC, WC], "cpu_thread_cnt": threads,
         "steps": steps, "ms_per_step_fed": fed * 1e3, "ms_in_next_per_step": in_next / steps * 1e3,
         "ms_in_next_augment_call": host["augment"] / steps * 1e3, "ms_in_next_issuing_copies": host["copy"] / steps * 1e3, "ms_per_step_resident": resident * 1e3, "fed_over_resident_rate": resident / fed}
    print(json.dumps(r), flush=True)
    return r


def rocprof_medians(db, iters, names=("plain_crop", "drawn", "worst")):
    """Median / min / max of the augment launches of a `--kernel --iters N` run under rocprofv3 (3 warm-up launches per set)."""
    import sqlite3
    rows = sqlite3.connect(db).execute("select name, start, end from kernels order by start").fetchall()
    us = [(e - s) / 1e3 for n, s, e in rows if "augment_kernel" in n]
    out = {}
    for k, name in enumerate(names):
        seg = us[k * (iters + 3) + 3:(k + 1) * (iters + 3)]
        out[name] = {"median_us": float(np.median(seg)), "min_us": float(min(seg)), "max_us": float(max(seg)), "launches": len(seg)}
    return out


def write_profile(prefix, res):
    with open(prefix + ".json", "w") as f:
        json.dump(res, f, indent=1)
    md = ["# Training feed on one MI355X: the augmentation kernel and the fed step", "",
          "Written by `tools/train_feed_time.py --profile` (numbers: `%s.json`)." % os.path.basename(prefix), ""]
    if "kernel" in res:
        rp = res.get("kernel_rocprofv3", {})
        md += ["## `byolo_augment_batch`, B = 8, 1024 x 1920 frames to 768 x 1440", "",
               "| plans | rocprofv3 median (min - max), us | device events median, us | bytes read (at least) / written |",
               "|---|---|---|---|"]
        for name, r in res["kernel"].items():
            p = rp.get(name)
            md.append("| %s | %s | %.1f | %.1f MB / %.1f MB |" % (
                name, "%.1f (%.1f - %.1f)" % (p["median_us"], p["min_us"], p["max_us"]) if p else "-", r["us_median"],
                r["min_bytes_read"] / 1e6, r["bytes_written"] / 1e6))
        md.append("")
    if "feed" in res:
        md += ["## Fed loop against resident batches (host wall time per step)", "",
               "| workload | cpu_thread_cnt | fed ms / step | resident ms / step | fed / resident | host ms in next(): total / event wait + augment launch / "
               "issuing copies |", "|---|---|---|---|---|---|"]
        for r in res["feed"]:
            md.append("| %s B=%d | %d | %.2f | %.2f | %.3f | %.2f / %.2f / %.2f |" % (
                r["variant"], r["B"], r["cpu_thread_cnt"], r["ms_per_step_fed"], r["ms_per_step_resident"], r["fed_over_resident_rate"],
                r["ms_in_next_per_step"], r["ms_in_next_augment_call"], r["ms_in_next_issuing_copies"]))
        md.append("")
    notes = ""                                       # hand-written reading of the numbers, kept across runs
    if os.path.exists(prefix + ".md"):
        old = open(prefix + ".md").read()
        if NOTES in old:
            notes = old[old.index(NOTES):]
    with open(prefix + ".md", "w") as f:
        f.write("\n".join(md) + ("\n" + notes if notes else ""))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--feed", action="store_true")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--threads", type=int, nargs="+", default=[16])
    ap.add_argument("--only", choices=sorted(WORKLOADS))
    ap.add_argument("--shards", help="folder for the generated shards (default: a temporary folder)")
    ap.add_argument("--json")
    ap.add_argument("--rocprof-db")
    ap.add_argument("--profile", help="write <PROFILE>.json and <PROFILE>.md")
    a = ap.parse_args()
    res = {}
    if a.kernel:
        res["kernel"] = kernel(a.iters)
    if a.feed:
        folder = a.shards or tempfile.mkdtemp(prefix="byolo_feed_")
        res["feed"] = [feed(n, a.steps, a.warmup, t, folder) for t in a.threads for n in ("yolov3", "bayes") if a.only in (None, n)]
    if a.rocprof_db:
        res["kernel_rocprofv3"] = rocprof_medians(a.rocprof_db, 20)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
    if a.profile:
        write_profile(a.profile, res)


if __name__ == "__main__":
    main()
