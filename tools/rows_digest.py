#!/usr/bin/env python
"""Digest of everything a forward hands out, for bit-for-bit A/B of two builds of libbyolo (BYOLO_LIB=...): SHA-256 of the pre-NMS
rows, the kept rows / indices / counts and the raw detection outputs, for each reference model at 64 x 96 (golden weights, dropout
on) and the Bayesian model at a benchmark-like shape (320 x 320, T = 6, 3 images: Winograd, fused pairs, 1x1 loop all in the plan).

Then the Bayesian model once per plan-option case of CASES, at both shapes -- one case per kernel family that takes an epilogue
descriptor (csrc/byolo_kernels.h EpiArgs) -- each with the counter hash, without dropout and with injected masks.  Every line ends
with the set of launch variants of one profiled forward (Engine.step_profile), and a case whose plan does not hold the variant it is
there for says MISSING and makes the exit status 1.

    BYOLO_LIB=$PWD/bayesian-yolov3_amd/byolo/libbyolo_ref.so python tools/rows_digest.py > a.txt; python tools/rows_digest.py > b.txt; diff a.txt b.txt
"""
import hashlib
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "bayesian-yolov3_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))

VARIANT = "bayesian_yolov3_aleatoric"
F32 = {"BYOLO_PRECISION": "f32"}
SPLIT = {"BYOLO_PRECISION": "split"}
WINO_SPLIT = dict(SPLIT, BYOLO_WINO_SPLIT="2", BYOLO_WINO_SPLIT_MIN_C="128", BYOLO_WINO_SPLIT_MIN_GFLOP="0")
# (name, environment of the new handle, launch variants the hash forward must hold at 64 x 96 / at 320 x 320, variants it must not)
# variants: 130 fused Winograd, 129 / 131 / 132 streaming GEMM (Winograd domain / 1x1 128-wide / 64-wide), -2 / -3 fp32 Winograd
# transforms, 4256 back-to-back pair, 140 / -4 split Winograd and its transform, -5 finish of an upsampled 1x1
CASES = [
    ("split default", SPLIT, (set(), set()), set()),
    ("f32 default", F32, (set(), set()), set()),
    ("f32 wino fused", dict(F32, BYOLO_WINOGRAD="2", BYOLO_WINO_FUSED="2"), ({130, -2}, {130, -2}), set()),
    ("f32 wino", dict(F32, BYOLO_WINOGRAD="2", BYOLO_WINO_FUSED="0"), ({129, -2, -3}, {129, -2, -3}), {130}),
    ("f32 wino fused igemm", dict(F32, BYOLO_WINOGRAD="2", BYOLO_WINO_FUSED="2", BYOLO_GEMM_STREAM="0"), ({130}, {130}), {129}),
    ("f32 wino igemm", dict(F32, BYOLO_WINOGRAD="2", BYOLO_WINO_FUSED="0", BYOLO_GEMM_STREAM="0"), ({-2, -3}, {-2, -3}), {129, 130}),
    ("f32 stream1x1", dict(F32, BYOLO_STREAM1X1="2"), ({131}, {131}), set()),
    ("split b2b 0", dict(SPLIT, BYOLO_B2B="0"), (set(), set()), {4256}),
    ("split b2b 2", dict(SPLIT, BYOLO_B2B="2"), ({4256}, {4256}), set()),
    ("split wino feed 0", dict(WINO_SPLIT, BYOLO_WINO_SPLIT_FEED="0"), ({140, -4, -5}, {140, -4, -5}), set()),
    ("split wino feed 3", dict(WINO_SPLIT, BYOLO_WINO_SPLIT_FEED="3"), ({140, -4}, {140, -4}), set()),
]
KNOBS = sorted({k for _, env, _, _ in CASES for k in env} | {"BYOLO_WINO_SPLIT_CHUNK_MB"})


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()[:24]


def out_digest(m, out):
    return digest(*[out[k].cpu().numpy() for k in ("boxes", "rows", "kept", "count")] + [dl.raw_output.cpu().numpy() for dl in m.det_layers])


def run_case(name, env, m, x, B, T, want, never):
    """hash / no dropout / injected masks: a profiled forward, then two plain ones (the second replays the captured graph)"""
    import torch
    eng = m.engine
    rng = np.random.default_rng(20261019)
    layout, _ = eng.mask_layout(B, T)
    bits = torch.from_numpy(eng.pack_masks([rng.random(n) < 0.9 for _, n in layout], B, T).view(np.int32)).cuda()
    ok = True
    for what, kw in (("hash", {}), ("no dropout", {"dropout_on": False}), ("injected", {"mask_bits": bits})):
        eng.set_profiling(2)
        d0 = out_digest(m, eng.forward(x, T=T, seed=42, want_boxes=True, **kw))
        variants = sorted({s["variant"] for s in eng.step_profile()})
        eng.set_profiling(0)
        eng.forward(x, T=T, seed=42, want_boxes=True, **kw)
        d1 = out_digest(m, eng.forward(x, T=T, seed=42, want_boxes=True, **kw))
        torch.cuda.synchronize()
        note = ""
        if what == "hash" and (not want <= set(variants) or never & set(variants)):
            note, ok = " MISSING %s / unexpected %s" % (sorted(want - set(variants)), sorted(never & set(variants))), False
        print("%-22s %dx%d T=%d B=%d %-10s" % (name, x.shape[1], x.shape[2], T, B, what), d0, d1, eng.precision, variants, note, flush=True)
    return ok


def main():
    import torch
    from conftest import build_model, golden_params, golden_images
    from byolo import synth
    for v in ("yolov3", "yolov3_aleatoric", "bayesian_yolov3_aleatoric"):
        B = 2
        _, m = build_model(v, 64, 96, T=3, params=golden_params(v), engine_options={"keep_all_outputs": True})
        m.finalize()
        out = m.run(torch.from_numpy(golden_images(B)).cuda(), seed=42)
        torch.cuda.synchronize()
        raws = [dl.raw_output.cpu().numpy() for dl in m.det_layers]
        print(v, "64x96", digest(out["boxes"].cpu().numpy()), digest(out["rows"].cpu().numpy(), out["kept"].cpu().numpy(), out["count"].cpu().numpy()),
              digest(*raws), digest(m.engine.layer_output(36).cpu().numpy(), m.engine.layer_output(74).cpu().numpy()))
    v = VARIANT
    for (H, W, T, B) in ((320, 320, 6, 3), (416, 416, 4, 2)):
        _, m = build_model(v, H, W, T=T)
        eng = m.engine
        eng.set_params(synth.base_params(eng.param_shapes(), v, 2, seed=7))
        eng.finalize()
        x = torch.from_numpy(synth.synthetic_images(B, H, W, seed=1234)).cuda()
        eng.calibrate_bn(x[:2])
        out = eng.forward(x, T=T, seed=42, want_boxes=True, want_nms=True)
        torch.cuda.synchronize()
        print(v, "%dx%d T=%d B=%d" % (H, W, T, B), digest(out["boxes"].cpu().numpy()),
              digest(out["rows"].cpu().numpy(), out["kept"].cpu().numpy(), out["count"].cpu().numpy()), eng.precision)
        eng.close()
    ok = True
    saved = {k: os.environ.get(k) for k in KNOBS}
    for name, env, (want_small, want_big), never in CASES:
        for k in KNOBS:
            os.environ.pop(k, None)
        os.environ.update(env)                                  # (the environment fills the plan options of a NEW handle)
        # 64 x 96, golden weights; the split Winograd in chunks of V that start and end inside an image (tests/test_gpu_wino_feed.py)
        if "BYOLO_WINO_SPLIT" in env:
            os.environ["BYOLO_WINO_SPLIT_CHUNK_MB"] = "0.12"
        _, m = build_model(v, 64, 96, T=3, params=golden_params(v))
        m.finalize()
        ok &= run_case(name, env, m, torch.from_numpy(golden_images(2)).cuda(), 2, 3, want_small, never)
        m.engine.close()
        os.environ.pop("BYOLO_WINO_SPLIT_CHUNK_MB", None)
        # 320 x 320, T = 6, 3 images: synthetic weights, BN calibrated on the device by this build
        _, m = build_model(v, 320, 320, T=6)
        m.engine.set_params(synth.base_params(m.engine.param_shapes(), v, 2, seed=7))
        m.engine.finalize()
        x = torch.from_numpy(synth.synthetic_images(3, 320, 320, seed=1234)).cuda()
        m.engine.calibrate_bn(x[:2])
        ok &= run_case(name, env, m, x, 3, 6, want_big, never)
        m.engine.close()
    for k, val in saved.items():
        os.environ.pop(k, None)
        if val is not None:
            os.environ[k] = val
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
