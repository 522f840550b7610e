#!/usr/bin/env python
"""Time the MC sample-count ladder (byolo_forward_ladder) at the headline shape -- 608 x 608, 8 images, T = 30, 2 classes, rungs
5, 10, 20, 30 -- beside the decode stage of the forward it reads, on the same handle in the same process, and write the figures
into the timing section of profiles/t_ladder.md (between its two marker lines; the rest of the file is left alone).

Device events throughout.  After a warm-up every repetition runs one profiled forward (byolo_stage_ms: the forward's own decode
stage and the four stages that make its step) and, behind it, one ladder between two events of its own; then the ladder once more
as a train of back-to-back calls between ONE pair of events, which takes the events' own cost out of a call this short.  Medians
with their spread (min .. max), the clocks the device reports before and after, and the bytes the ladder moves over its time.

    python tools/t_ladder_time.py [--reps 30] [--train 50] [--out profiles/t_ladder.md]
"""
import argparse
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "bayesian-yolov3_amd"))

BEGIN, END = "<!-- t_ladder_time.py: begin -->", "<!-- t_ladder_time.py: end -->"
VARIANT, H, W, B, T, C = "bayesian_yolov3_aleatoric", 608, 608, 8, 30, 2
RUNGS = [5, 10, 20, 30]


def clocks():
    """The clock lines of `rocm-smi --showclocks` for the first device (a read-only query), or a note that there are none."""
    try:
        out = subprocess.run(["rocm-smi", "--showclocks", "-d", "0"], capture_output=True, text=True, timeout=60).stdout
    except Exception as e:                                     # noqa: BLE001 -- a note in the profile, not a failure of the timing
        return "not read (%s)" % e
    lines = [l.split(":", 1)[1].strip() for l in out.splitlines() if "clock level" in l and ("sclk" in l or "mclk" in l or "fclk" in l)]
    return "; ".join(lines) if lines else "not reported"


def spread(xs):
    return "%.4f (min %.4f, max %.4f, n %d)" % (statistics.median(xs), min(xs), max(xs), len(xs))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--train", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "t_ladder.md"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("t_ladder_time.py measures on the device: no GPU here, nothing is written")
    from byolo import synth
    from lib_yolo import model, yolov3
    config = {"full_img_size": [H, W, 3], "crop": False, "cls_cnt": C, "priors": yolov3.ECP_9_PRIORS, "aleatoric_loss": False,
              "inference_mode": True, "T": T, "implicit_background_class": True}
    m = getattr(yolov3, VARIANT)(config).init_model(inputs=model.Placeholder((None, H, W, 3)), training=False).get_model()
    eng = m.engine
    eng.set_params(synth.base_params(eng.param_shapes(), VARIANT, C, seed=7))
    eng.finalize()
    eng.calibrate_bn(torch.from_numpy(synth.synthetic_images(2, H, W, seed=999)).cuda())
    x = torch.from_numpy(synth.synthetic_images(B, H, W, seed=1234)).cuda()
    N, D = eng.num_boxes()
    slabs = torch.empty((len(RUNGS), B, N, D), device="cuda")
    keep = None
    clk0 = clocks()
    eng.set_profiling(1)
    for _ in range(args.warmup):
        keep = eng.forward(x, T=T, seed=42, want_boxes=True, out=keep)
        eng.t_ladder(RUNGS, B, T, out=slabs)
    torch.cuda.synchronize()
    assert torch.equal(slabs[-1].view(torch.int32), keep["boxes"].view(torch.int32)), "rung T is not the forward's decode"
    ladder, decode, step = [], [], []
    for _ in range(args.reps):
        keep = eng.forward(x, T=T, seed=42, want_boxes=True, out=keep)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        eng.t_ladder(RUNGS, B, T, out=slabs)
        e1.record()
        torch.cuda.synchronize()
        st = eng.stage_ms()
        ladder.append(e0.elapsed_time(e1))
        decode.append(st["decode"])
        step.append(sum(st.values()))
    eng.set_profiling(0)
    trains = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.train):
            eng.t_ladder(RUNGS, B, T, out=slabs)
        e1.record()
        torch.cuda.synchronize()
        trains.append(e0.elapsed_time(e1) / args.train)
    clk1 = clocks()
    cells = sum(dl.h * dl.w for dl in m.det_layers)
    pitch = -(-3 * 2 * (5 + C) // 4) * 4                       # a detection head's rows are padded to a multiple of 4 floats
    read = cells * B * T * pitch * 4                           # every launch reads whole cells: the std logits ride along in the lines
    written = len(RUNGS) * B * N * D * 4
    ml, md, ms, mt = (statistics.median(v) for v in (ladder, decode, step, trains))
    lines = [BEGIN,
             "Measured by `tools/t_ladder_time.py` on %s: %s, %d x %d, %d images, T = %d, %d classes, rungs %s, precision %s." % (
                 torch.cuda.get_device_name(0), VARIANT, H, W, B, T, C, RUNGS, eng.precision),
             "Device events; %d warm-up rounds, then %d rounds of one profiled forward and one ladder behind it. Milliseconds, median (spread)." % (args.warmup, args.reps),
             "",
             "| what | ms |", "|---|---|",
             "| `byolo_forward_ladder`, one call between two events | %s |" % spread(ladder),
             "| `byolo_forward_ladder`, per call in a train of %d between two events (5 trains) | %s |" % (args.train, spread(trains)),
             "| the same forwards' decode stage (`byolo_stage_ms`) | %s |" % spread(decode),
             "| the same forwards' step (the four stages of `byolo_stage_ms`) | %s |" % spread(step),
             "",
             "- ladder / decode stage: %.2f (single calls), %.2f (train)" % (ml / md, mt / md),
             "- the ladder's share of the measured step: %.2f %% (single calls), %.2f %% (train)" % (100 * ml / ms, 100 * mt / ms),
             "- the ladder reads %.1f MB of raw detection outputs (%d cells x %d samples x %d floats) and writes %.1f MB of rows: "
             "%.0f GB/s over the train's time" % (read / 1e6, cells, B * T, pitch, written / 1e6, (read + written) / mt / 1e6),
             "- clocks before: %s" % clk0, "- clocks after: %s" % clk1, END]
    text = open(args.out).read() if os.path.exists(args.out) else ""
    block = "\n".join(lines)
    if BEGIN in text and END in text:
        text = text[:text.index(BEGIN)] + block + text[text.index(END) + len(END):]
    else:
        text = text + ("\n" if text and not text.endswith("\n") else "") + block + "\n"
    with open(args.out, "w") as f:
        f.write(text)
    print(block)
    eng.close()


if __name__ == "__main__":
    main()
