"""The decode and MC-reduction kernels (csrc/tail_kernels.hip) against FLOAT64, stage by stage, through Engine.decode and
Engine.epistemic_stats: every build (exact and capacity class counts, both sides of each capacity boundary), the grid-stride
loop's second trip, epi_stats_kernel with every output combination, and the T-shard modes in the capacity builds.

Inputs, reference and assertion are tests/_decode_ref.py's; tests/test_decode_f64_cpu.py shows on the CPU that the inputs need no
exclusion, that the float32 oracle passes the same `check_rows`, and that ten wrong kernels fail it.  The contract is
oracle/report.py's as it stands -- device vs float64 at allowance(floor), vs float32 at allowance(floor, "float32"), ids exact,
NaN / inf patterns equal -- and every distance goes to the parity table (conftest.record_parity).  Measured numbers:
profiles/decode_f64.md."""
import ctypes
import time

import numpy as np
import pytest

import _decode_ref as R
from conftest import assert_close, assert_rows_close, build_model, golden_images, golden_params, record_parity, rows_report
from oracle.report import allowance

pytestmark = pytest.mark.gpu


def _torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def engine():
    """Engine(cls_cnt) per class count, made once: the staged entry points read nothing of a handle but its class count."""
    from byolo import Engine
    made = {}

    def get(C):
        if C not in made:
            made[C] = Engine((64, 64, 3), C)
        return made[C]
    yield get
    for e in made.values():
        e.close()


def _decode(eng, c, raw):
    torch = _torch()
    buf = torch.full((c.B, R.n_total(c), R.geometry(c)[2]), float(R.SENTINEL), device="cuda")
    eng.decode(c.kind, torch.tensor(raw, device="cuda"), c.B, c.T, R.PRIORS, c.layer_id, buf, c.box_base)
    torch.cuda.synchronize()
    return buf.cpu().numpy()


def _note(what, **kv):
    """A measurement that is no distance: printed, and filed in the parity table under its own key."""
    print("%s: %s" % (what, ", ".join("%s %.4g" % i for i in kv.items())))
    record_parity(what, {k: dict(worst_in_bounds=float(v), max_abs_err=float(v), max_ref=0.0) for k, v in kv.items()}, kind="note")


@pytest.mark.parametrize("c", R.build_cases(), ids=R.case_id)
def test_every_build(engine, c):
    """Kinds 0 .. 2 x the exact builds (C = 1, 2, 3, 4, 8, 80) and the capacity builds (5 | 9, 24 | 25, 48 | 49, 81, 128), B = 2 on
    a 5 x 7 grid: spread (T = 7 for kind 2), and for kind 2 also agree (T = 50) and one pass (T = 1).

    T = 1: the float64 covariance and determinant are exactly 0; the device's `s_ll / T - ev * ev` is a contracted multiply-add of
    the ROUNDED square and the exact one, i.e. the rounding error of l * l with either sign -- inside the contract (an ulp of l^2),
    but a NEGATIVE epistemic variance is what var_recal's power map and the sigma of the JSON writers would read.  The largest
    |variance| and the most negative one are recorded (profiles/decode_f64.md), not clamped."""
    ref = R.reference(c)
    got = _decode(engine(c.C), c, ref["raw"])
    rep = R.check_rows(c, got, ref, "decode f64 %s" % R.case_id(c))
    record_parity("decode f64 %s: float32 oracle vs float64 oracle (the floor)" % R.case_id(c), ref["floor"])
    print("%s: device vs float64 %.4f | device vs float32 %.4f | float32 vs float64 %.4f (worst group, units of the bound)"
          % (R.case_id(c), R.worst(rep["f64"]), R.worst(rep["f32"]), R.worst(ref["floor"])))
    if c.kind == 2 and c.T == 1:
        assert not ref["r64"][..., 4:8].any() and not ref["r64"][..., 12].any()
        var = got[:, c.box_base:c.box_base + R.n_rows(c), 4:8].astype(np.float64)
        _note("decode f64 %s: epistemic variance of a single pass" % R.case_id(c), max_abs=np.abs(var).max(), most_negative=var.min(),
              negative_elements=float((var < 0).sum()))


@pytest.mark.parametrize("c", R.stride_cases(), ids=R.case_id)
def test_grid_stride_second_trip(engine, c):
    """More lanes than launch_decode_c's largest grid (4096 x 256): 2 x 421 x 419 x 3 = 1 058 394, so the last 9 818 lanes --
    image 1's final cells, the -800 plant among them -- are the loop's second trip, which no shipped workload takes (the largest,
    1024 x 1920 batch 11 at stride 8, has 1 013 760 lanes).  The whole buffer is held to the float64 reference; the host time of
    that reference is printed and recorded, it is what bounds this case's duration."""
    assert c.B * c.lh * c.lw * 3 > R.STRIDE_LANES
    t0 = time.time()
    ref = R._reference(c)                                          # not cached: hundreds of MB
    t1 = time.time()
    got = _decode(engine(c.C), c, ref["raw"])
    t2 = time.time()
    what = "decode f64 grid-stride %s" % R.case_id(c)
    rep = R.check_rows(c, got, ref, what)
    t3 = time.time()
    record_parity(what + ": float32 oracle vs float64 oracle (the floor)", ref["floor"])
    # the second trip on its own (it is inside the check above; this is the figure for the profile note)
    n2 = c.B * c.lh * c.lw * 3 - R.STRIDE_LANES
    lanes = np.arange(R.STRIDE_LANES, R.STRIDE_LANES + n2)
    pr, cell = lanes % 3, (lanes // 3) % (c.lh * c.lw)
    assert ((lanes // 3) // (c.lh * c.lw) == c.B - 1).all()
    idx = pr * (c.lh * c.lw) + cell
    g2 = got[c.B - 1, c.box_base:c.box_base + R.n_rows(c)][idx]
    if c.kind == 2:
        g2 = g2.copy()
        g2[..., 12] = 0
    b, row, col, ppr, _ = R.plant_lanes(c)[-1]                     # the -800 plant (all finite for kind 0: no entropy there)
    assert b == c.B - 1 and ppr * (c.lh * c.lw) + row * c.lw + col in idx and len(idx) > 1, "the second trip holds a plant and ordinary lanes"
    assert c.kind == 0 or not np.isfinite(ref["z64"][c.B - 1][idx]).all()
    rep2 = rows_report(g2, ref["z64"][c.B - 1][idx], R.VARIANTS[c.kind], c.C)
    record_parity(what + ": second trip alone vs the float64 oracle", rep2)
    _note(what + ": host seconds", reference=t1 - t0, device_and_copies=t2 - t1, comparison=t3 - t2)
    print("%s: device vs float64 %.4f (second trip alone %.4f) | vs float32 %.4f | floor %.4f"
          % (what, R.worst(rep["f64"]), R.worst(rep2), R.worst(rep["f32"]), R.worst(ref["floor"])))


# ---------------------------------------------------------------------------------------------
# epi_stats_kernel
# ---------------------------------------------------------------------------------------------
def _stats_reference(c, raw, dtype):
    """decode_epistemic_stats per image plus the per-sample sigmoid / softmax, in `dtype`: the four outputs of the kernel."""
    torch = _torch()
    from oracle import cpu_ref
    rt = torch.from_numpy(raw).to(dtype)
    with torch.no_grad():
        st = [cpu_ref.decode_epistemic_stats(rt[b * c.T:(b + 1) * c.T], c.C) for b in range(c.B)]
        d = rt.reshape(c.B * c.T, c.lh, c.lw, 3, 2 * (5 + c.C))
        return dict(ev_loc=torch.stack([s["ev_loc"] for s in st]).numpy(), epi_covar_loc=torch.stack([s["epi_covar_loc"] for s in st]).numpy(),
                    obj_samples=torch.sigmoid(d[..., 8]).numpy(), cls_samples=torch.softmax(d[..., 10:10 + c.C], dim=-1).numpy())


STATS_KEYS = ("ev_loc", "epi_covar_loc", "obj_samples", "cls_samples")       # byolo_epistemic_stats' output order


def _check_stats(c, got, raw, what):
    """Each output within 1e-4 * max(1, |ref|) of float64 (conftest.assert_close: the contract's bound per value; the float32
    oracle's own distance is recorded beside it); the covariance symmetric bit for bit."""
    torch = _torch()
    r64, r32 = _stats_reference(c, raw, torch.float64), _stats_reference(c, raw, torch.float32)
    dist = {}
    for k in STATS_KEYS:
        g = got[k].cpu().numpy()
        assert np.isfinite(r64[k]).all() and np.isfinite(g).all(), k
        tol = np.maximum(R.RTOL, R.RTOL * np.abs(r64[k]))
        dist[k] = dict(device=float((np.abs(g - r64[k]) / tol).max()), float32=float((np.abs(r32[k] - r64[k]) / tol).max()))
        print("%s %s: device vs float64 %.4f | float32 vs float64 %.4f (units of the bound)" % (what, k, dist[k]["device"], dist[k]["float32"]))
        assert_close(g, r64[k], "%s %s vs float64" % (what, k))
        assert_close(g, r32[k], "%s %s vs float32" % (what, k))
    record_parity(what + " vs the float64 oracle", {k: dict(worst_in_bounds=v["device"], max_abs_err=0.0, max_ref=0.0) for k, v in dist.items()}, kind="stats")
    record_parity(what + ": float32 oracle vs float64 oracle (the floor)", {k: dict(worst_in_bounds=v["float32"], max_abs_err=0.0, max_ref=0.0) for k, v in dist.items()}, kind="stats")
    cov = got["epi_covar_loc"]
    assert torch.equal(cov.view(torch.int32), cov.transpose(-1, -2).contiguous().view(torch.int32)), "covariance not symmetric bit for bit"


@pytest.mark.parametrize("C", [2, 5, 24, 49, 128])
def test_epi_stats_every_build_and_output_combination(engine, C):
    """epi_stats_kernel's exact build (2) and its four capacity builds (8, 24, 48, 128 slots), B = 3 images, T = 7, grid 3 x 5,
    spread logits with the four plants: against float64; the covariance symmetric and its diagonal the decode kernel's columns
    4 .. 7, bit for bit; and byolo_epistemic_stats with each output NULL in turn -- the others keep their bits, and a guard of
    sentinels behind every output stays untouched."""
    torch = _torch()
    from byolo._lib import lib, check
    c = R.make_case(2, C, B=3, T=7, lh=3, lw=5)
    raw = R.make_raw(c)
    eng = engine(C)
    d_raw = torch.from_numpy(raw).cuda()
    what = "epi_stats f64 C%d" % C
    full = eng.epistemic_stats(d_raw, c.B, c.T)
    torch.cuda.synchronize()
    _check_stats(c, full, raw, what)
    rows = torch.from_numpy(_decode(eng, c, raw)).cuda()[:, c.box_base:c.box_base + R.n_rows(c)]
    rows = rows.reshape(c.B, 3, c.lh, c.lw, -1).permute(0, 2, 3, 1, 4)                  # prior-major rows -> [B, lh, lw, 3, D]
    diag = torch.diagonal(full["epi_covar_loc"], dim1=-2, dim2=-1)
    assert torch.equal(diag.contiguous().view(torch.int32), rows[..., 4:8].contiguous().view(torch.int32)), "diagonal != the row's columns 4 .. 7"

    GUARD = 64
    sent = float(R.SENTINEL)
    stream = ctypes.c_void_p(torch.cuda.current_stream(d_raw.device).cuda_stream)
    for null in (None,) + STATS_KEYS:
        bufs = {k: torch.full((full[k].numel() + GUARD,), sent, device="cuda") for k in STATS_KEYS}
        ptr = [ctypes.c_void_p(None if k == null else bufs[k].data_ptr()) for k in STATS_KEYS]
        check(eng._h, lib.byolo_epistemic_stats(eng._h, ctypes.c_void_p(d_raw.data_ptr()), c.B, c.T, c.lh, c.lw, *ptr, stream))
        torch.cuda.synchronize()
        for k in STATS_KEYS:
            n = full[k].numel()
            assert (bufs[k][n:] == sent).all(), "output %s NULL: guard behind %s written" % (null, k)
            if k == null:
                assert (bufs[k] == sent).all()
            else:
                assert torch.equal(bufs[k][:n].view(torch.int32), full[k].reshape(-1).view(torch.int32)), \
                    "output %s NULL: %s changed its bits" % (null, k)


def test_epi_stats_grid_stride_second_trip(engine):
    """epi_stats_kernel's own grid cap (launch_epi_stats_c: 4096 x 256) with the same 2 x 421 x 419 x 3 lanes, C = 2, T = 2."""
    torch = _torch()
    c = R.make_case(2, 2, T=2, **R.STRIDE_GRID)
    assert c.B * c.lh * c.lw * 3 > R.STRIDE_LANES
    t0 = time.time()
    raw = R.make_raw(c)
    got = engine(2).epistemic_stats(torch.from_numpy(raw).cuda(), c.B, c.T)
    torch.cuda.synchronize()
    t1 = time.time()
    _check_stats(c, got, raw, "epi_stats f64 grid-stride %s" % R.case_id(c))
    # the -800 plant sits in the second trip and is what it should be
    b, row, col, pr, _ = R.plant_lanes(c)[-1]
    assert (got["ev_loc"][b, row, col, pr] == -800).all() and (got["obj_samples"][b * c.T:(b + 1) * c.T, row, col, pr] == 0).all()
    _note("epi_stats f64 grid-stride %s: host seconds" % R.case_id(c), input_and_device=t1 - t0, reference_and_comparison=time.time() - t1)


# ---------------------------------------------------------------------------------------------
# T shards in the capacity builds
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shard_model():
    """One model per class count with its one-call rows and the float64 oracle's, shared by the shard sets."""
    made = {}

    def get(C):
        if C not in made:
            torch = _torch()
            from oracle import cpu_ref
            v, T = "bayesian_yolov3_aleatoric", 6
            params = golden_params(v, cls_cnt=C)                     # synth.base_params(seed 7) + the fixtures' BN statistics
            _, m = build_model(v, 64, 96, T=T, params=params, cls_cnt=C)
            m.finalize()
            imgs = golden_images(1)
            x = torch.from_numpy(imgs).cuda()
            whole = m.engine.forward(x, T=T, seed=42, want_boxes=True, want_nms=False)["boxes"].clone()
            with torch.no_grad():
                ref64, _ = cpu_ref.detect_boxes(cpu_ref.to_torch_params(params, torch.float64), imgs, v, T=T, seed=42, cls_cnt=C, dtype=torch.float64)
                ref32, _ = cpu_ref.detect_boxes(cpu_ref.to_torch_params(params), imgs, v, T=T, seed=42, cls_cnt=C)
            made[C] = dict(m=m, x=x, whole=whole, ref64=ref64.numpy(), ref32=ref32.numpy())
        return made[C]
    return get


@pytest.mark.parametrize("cuts", [((0, 1), (1, 2), (3, 3)), ((0, 6),)], ids=["1+2+3", "6"])
@pytest.mark.parametrize("C", [5, 80])
def test_t_shards_in_the_capacity_and_the_80_class_builds(shard_model, C, cuts):
    """test_gpu_parity.py::test_t_shards_add_up_to_the_whole_forward's scheme where the sums of modes 1 and 2 go through the masked
    loads and stores (`EXACT || c < C`: cls_cnt = 5 in the 8-slot capacity build) and through the widest exact build (80): T = 6
    samples of one 64 x 96 image cut into shards, each handing out its per-box sums, the sums added, byolo_finish_tshard.  One
    shard of all six is the one-call forward bit for bit; several are within the contract of the one-call rows and of the float64
    oracle, ids exact."""
    torch = _torch()
    v, T = "bayesian_yolov3_aleatoric", 6
    s = shard_model(C)
    eng = s["m"].engine
    sums = None
    for t0, tl in cuts:
        part = eng.forward(s["x"], T=tl, seed=42, want_boxes=True, want_nms=False, t_shard=(t0, T))["boxes"]
        sums = part.clone() if sums is None else sums + part
    rows = eng.finish_tshard(sums.contiguous(), T)
    torch.cuda.synchronize()
    got, ref = rows.cpu().numpy(), s["whole"].cpu().numpy()
    what = "T shards C%d %s" % (C, "+".join(str(tl) for _, tl in cuts))
    if len(cuts) == 1:
        assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), "one shard of all samples must be the one-call forward bit for bit"
    assert_rows_close(got, ref, v, what + " vs the one-call forward", C=C)
    floor = rows_report(s["ref32"], s["ref64"], v, C)
    record_parity(what + ": float32 oracle vs float64 oracle (the floor)", floor)
    assert_rows_close(got, s["ref64"], v, what + " vs the float64 oracle", C=C, allowed=allowance(floor))
    again = eng.forward(s["x"], T=T, seed=42, want_boxes=True, want_nms=False)["boxes"]
    assert torch.equal(again, s["whole"]), "the handle is back in the normal mode afterwards"
