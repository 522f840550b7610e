"""The MC sample-count ladder (include/byolo.h "MC sample-count ladder"): decode_epi_ladder_kernel through Engine.decode_ladder,
byolo_forward_ladder through Engine.t_ladder, the evaluation's rung_tail helper and the `t_ladder` key of evaluate.py.

The contract is BIT IDENTITY with decode_epi_kernel -- the kernel tests/test_decode_f64_gpu.py holds to float64 -- on each image's
first k samples: every comparison below is of int32 bit patterns (NaNs included; the generators of tests/_decode_ref.py plant
saturated objectness and +-800 logits, so the entropies of those lanes are NaN).  There is no tolerance in this file."""
import ctypes
import json

import numpy as np
import pytest
import torch

import _decode_ref as R
import _var_recal_ref as vr

pytestmark = pytest.mark.gpu

VARIANT = "bayesian_yolov3_aleatoric"
SENT = float(R.SENTINEL)
EXACT_C = (1, 2, 3, 4, 8)                         # launch_decode_ladder's exact builds
CAPACITY_C = (5, 9, 24, 25, 48)                   # its capacity builds (8 / 24 / 48 slots), both sides of each boundary
LIMIT = 48                                        # BYOLO_T_LADDER_MAX_CLASSES


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


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


def _first(raw, B, T, k):
    """The first k samples of every image of raw [B * T, lh, lw, F]."""
    return raw.view(B, T, *raw.shape[1:])[:, :k].contiguous().view(B * k, *raw.shape[1:])


def _staged(eng, c, rungs, raw=None):
    """decode_ladder into a sentinel-filled [K, B, n_total, D] against one Engine.decode per rung into a buffer filled alike:
    equal whole buffers say the rows are the decode's AND nothing outside box_base .. box_base + rows was written."""
    D = R.geometry(c)[2]
    raw = torch.from_numpy(R.make_raw(c)).cuda() if raw is None else raw
    got = torch.full((len(rungs), c.B, R.n_total(c), D), SENT, device="cuda")
    eng.decode_ladder(raw, c.B, c.T, R.PRIORS, c.layer_id, rungs, got, c.box_base)
    lo, hi = c.box_base, c.box_base + R.n_rows(c)
    for j, k in enumerate(rungs):
        want = torch.full((c.B, R.n_total(c), D), SENT, device="cuda")
        eng.decode(2, _first(raw, c.B, c.T, k), c.B, k, R.PRIORS, c.layer_id, want, c.box_base)
        assert torch.equal(_bits(got[j]), _bits(want)), "%s rung %d of %s" % (R.case_id(c), k, rungs)
        assert (got[j][:, :lo] == SENT).all() and (got[j][:, hi:] == SENT).all() and not (got[j][:, lo:hi, -1] == SENT).any()
    return got


@pytest.mark.parametrize("C", EXACT_C + CAPACITY_C)
def test_staged_every_build(engine, C):
    c = R.make_case(2, C)
    assert (c.B, c.T, c.lh, c.lw) == (2, 7, 5, 7)
    got = _staged(engine(C), c, [1, 2, 7])
    assert torch.isnan(got[:, :, c.box_base:c.box_base + R.n_rows(c)]).any(), "the plants make NaN entropies: they are compared too"
    assert not torch.equal(_bits(got[1]), _bits(got[2]))                  # the rungs are not one another


@pytest.mark.parametrize("T,rungs", [(7, [7]), (1, [1]), (7, list(range(1, 8))), (16, list(range(1, 17)))],
                         ids=["last-alone", "T1", "every-count", "16-rungs"])
def test_rung_patterns(engine, T, rungs):
    _staged(engine(2), R.make_case(2, 2, T=T), rungs)


def test_grid_stride_second_trip(engine):
    """More lanes than the launch's 4096 x 256, as R.stride_cases() does it: 2 x 421 x 419 x 3, C = 1, T = 2."""
    c = R.make_case(2, 1, T=2, **R.STRIDE_GRID)
    assert c.B * c.lh * c.lw * 3 > R.STRIDE_LANES
    _staged(engine(1), c, [1, 2])


# ---- from a forward -------------------------------------------------------------------------------------------------------------
def _model(engine_options=None, T=6, variant=VARIANT, H=64, W=96):
    from conftest import build_model, golden_params
    m = build_model(variant, H, W, T=T, B=2, params=golden_params(variant), engine_options=engine_options or {})[1]
    m.finalize()
    return m


def _images(B=2):
    from conftest import golden_images
    return torch.from_numpy(golden_images(B)).cuda()


def _var_cal(seed=5):
    from byolo.recalibrate import VarCalibration
    a, b = vr.table([3, 3, 3], rng=np.random.default_rng(seed), power=True)
    rows = lambda t: [[list(map(float, t[l][p])) for p in range(3)] for l in range(3)]
    return VarCalibration(VARIANT, [3, 3, 3], target="total", a=rows(a), b=rows(b))


def _score_cal(seed=23):
    from byolo.score_recal import ScoreCalibration
    rng = np.random.default_rng(seed)
    cal = ScoreCalibration(VARIANT, 2, None, "class")
    for g in range(cal.n_groups):
        cal.w[g] = [float(rng.normal(0.0, 0.5)), float(rng.uniform(0.5, 1.5))] + [float(v) for v in rng.normal(0.0, 0.2, cal.K - 2)]
    return cal


@pytest.mark.parametrize("precision", ["split", "f32"])
def test_from_a_forward(precision):
    B, T = 2, 6
    m = _model()
    x = _images(B)
    res = m.run(x, seed=42, want_boxes=True, precision=precision)
    eng = res["engine"]
    assert eng.precision == precision
    slabs = eng.t_ladder([2, 3, 6], B, T)
    assert slabs.shape == (3, B) + tuple(res["boxes"].shape[1:]) and slabs.device == res["boxes"].device
    assert torch.equal(_bits(slabs[2]), _bits(res["boxes"])), "the rung T is the forward's own decode"
    for j, k in ((0, 2), (1, 3)):
        want = torch.full_like(res["boxes"], SENT)
        for dl in m.det_layers:
            raw = eng.layer_output(dl._raw_ref.index)                     # dense [B * T, lh, lw, F]
            eng.decode(2, _first(raw, B, T, k), B, k, [(p.h, p.w) for p in dl.priors], dl.layer_id, want, dl._box_base)
        assert not (want[..., -1] == SENT).any()
        assert torch.equal(_bits(slabs[j]), _bits(want)), (precision, k)
    assert not torch.equal(_bits(slabs[0]), _bits(slabs[2]))
    # into a caller's buffer, and the same bits again (the forward's workspace is still there)
    out = torch.full_like(slabs, SENT)
    assert eng.t_ladder([2, 3, 6], B, T, out=out) is out and torch.equal(_bits(out), _bits(slabs))
    m.engine.close()


@pytest.mark.parametrize("precision", ["split", "f32"])
def test_from_a_forward_with_variance_recalibration(precision):
    B, T = 2, 6
    cal = _var_cal()
    m = _model({"var_recal": cal})
    res = m.run(_images(B), seed=42, want_boxes=True, precision=precision)
    eng = res["engine"]
    slabs = eng.t_ladder([2, 3, 6], B, T)
    assert torch.equal(_bits(slabs[2]), _bits(res["boxes"])), "a slab is what the forward hands its NMS: recalibrated"
    off = _model()                                                        # the same forward without the table: the raw rows
    plain = off.run(_images(B), seed=42, want_boxes=True, precision=precision)["engine"].t_ladder([2, 3, 6], B, T)
    assert not torch.equal(_bits(plain[2]), _bits(slabs[2]))
    assert torch.equal(_bits(eng.var_recal(plain, cal)), _bits(slabs)), "every slab is the stand-alone stage on the raw slab"
    # a setting that invalidates the handle's plan takes the ladder of the forward before it along
    from byolo import _lib
    eng.set_var_recal(None)
    with pytest.raises(_lib.ByoloError) as e:
        eng.t_ladder([2], B, T)
    assert e.value.code == _lib.ERR_STATE
    off.engine.close()
    m.engine.close()


# ---- the evaluation's tail helper ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("options", ["plain", "var_recal+box_vote", "soft_nms+score_recal"])
def test_tail_helper_at_rung_T_is_the_forward(options):
    """evaluate.rung_tail on the slab of rung T: kept rows, kept indices and counts (and vote counts / scores where those stages
    run) equal the forward's own, bit for bit -- the stand-alone stages in the forward's order are the fused tail."""
    import evaluate
    B, T = 2, 6
    opts = {"plain": {}, "var_recal+box_vote": {"var_recal": _var_cal(), "box_vote": {"sigma_t": 0.05}},
            "soft_nms+score_recal": {"soft_nms": {"method": "linear", "iou_soft": 0.2}, "score_recal": _score_cal()}}[options]
    m = _model(opts)
    res = m.run(_images(B), seed=42, want_boxes=True)
    eng = res["engine"]
    slab = eng.t_ladder([3, T], B, T)[1]
    got = evaluate.rung_tail(eng, m, slab)
    keys = ["rows", "kept", "count"] + (["vote_n"] if "box_vote" in opts else []) + (["score"] if "score_recal" in opts else [])
    assert int(res["count"][:, 0].min()) > 0
    for k in keys:
        assert torch.equal(_bits(got[k]), _bits(res[k])), (options, k)
    low = evaluate.rung_tail(eng, m, eng.t_ladder([3, T], B, T)[0])
    assert not torch.equal(_bits(low["rows"]), _bits(res["rows"]))        # three samples keep other rows than six
    m.engine.close()


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def _ladder_rc(eng, B, T, rungs, out):
    from byolo import _lib
    arr = (ctypes.c_int32 * max(1, len(rungs)))(*rungs)
    rc = _lib.lib.byolo_forward_ladder(eng._h, B, T, arr, len(rungs), ctypes.c_void_p(out.data_ptr()),
                                       ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    return rc, _lib.lib.byolo_last_error(eng._h).decode()


def test_refusals():
    from byolo import Engine, _lib
    B, T = 2, 6
    m = _model()
    eng = m.engine
    N, D = eng.num_boxes()
    out = torch.full((17, B, N, D), SENT, device="cuda")
    rc, msg = _ladder_rc(eng, B, T, [2, 6], out)
    assert rc == _lib.ERR_STATE and "no forward has run" in msg
    m.run(_images(B), seed=42, want_boxes=True)
    assert _ladder_rc(eng, B, T, [2, 6], out)[0] == _lib.OK
    torch.cuda.synchronize()
    out.fill_(SENT)
    for b, t in ((B + 1, T), (B - 1, T), (B, T - 1), (B, T + 1)):
        rc, msg = _ladder_rc(eng, b, t, [1], out)
        assert rc == _lib.ERR_ARG and "the workspace holds a forward of (2, 6)" in msg, (b, t, msg)
    for rungs, word in (([3, 2], "strictly increasing"), ([2, 2], "strictly increasing"), ([0, 2], "outside 1 .. T"), ([2, 7], "outside 1 .. T"),
                        ([-1], "outside 1 .. T"), (list(range(1, 18)), "1 .. 16 rungs"), ([], "1 .. 16 rungs")):
        rc, msg = _ladder_rc(eng, B, T, rungs, out)
        assert rc == _lib.ERR_ARG and word in msg, (rungs, msg)
        with pytest.raises(ValueError) as e:                              # the binding refuses in the library's words
            eng.t_ladder(rungs, B, T)
        assert str(e.value) == msg, (rungs, str(e.value), msg)
    assert _lib.lib.byolo_set_tshard(eng._h, 0, T) == 0                   # a T shard set on the handle
    rc, msg = _ladder_rc(eng, B, T, [2, 6], out)
    assert rc == _lib.ERR_ARG and "T shard" in msg
    assert _lib.lib.byolo_set_tshard(eng._h, 0, 0) == 0
    torch.cuda.synchronize()
    assert (out == SENT).all(), "a refused call launches nothing"
    assert _ladder_rc(eng, B, T, [2, 6], out)[0] == _lib.OK              # ... and leaves the handle usable
    eng.close()

    ale = _model(T=1, variant="yolov3_aleatoric")                         # aleatoric detection layers have no samples to walk
    ale.run(_images(B), seed=42, want_boxes=True)
    N, D = ale.engine.num_boxes()
    buf = torch.full((1, B, N, D + 7), SENT, device="cuda")
    rc, msg = _ladder_rc(ale.engine, B, 1, [1], buf)
    torch.cuda.synchronize()
    assert rc == _lib.ERR_ARG and "epistemic" in msg and (buf == SENT).all()
    ale.engine.close()

    big = Engine((64, 64, 3), LIMIT + 1)                                  # more classes than the largest scratch-free build
    c = R.make_case(2, LIMIT + 1)
    raw = torch.from_numpy(R.make_raw(c)).cuda()
    buf = torch.full((1, c.B, R.n_total(c), R.geometry(c)[2]), SENT, device="cuda")
    pri = (ctypes.c_float * 6)(*[float(v) for p in R.PRIORS for v in p])
    rc = _lib.lib.byolo_decode_ladder(big._h, ctypes.c_void_p(raw.data_ptr()), c.B, c.T, c.lh, c.lw, pri, c.layer_id, (ctypes.c_int32 * 1)(7), 1,
                                      ctypes.c_void_p(buf.data_ptr()), R.n_total(c), c.box_base, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    msg = _lib.lib.byolo_last_error(big._h).decode()
    torch.cuda.synchronize()
    assert rc == _lib.ERR_ARG and "at most %d classes" % LIMIT in msg and (buf == SENT).all()
    with pytest.raises(ValueError, match="at most %d classes" % LIMIT):
        big.decode_ladder(raw, c.B, c.T, R.PRIORS, c.layer_id, [7], buf, c.box_base)
    big.close()


def test_a_forward_cut_into_pieces_has_no_ladder():
    """A batch beyond byolo_max_images(T) runs as pieces in one workspace, which then holds the LAST piece: refused (the plan's batch
    is the piece's).  608 x 608 at T = 1 is the cheapest shape at which a batch exceeds one call's capacity."""
    from conftest import build_model
    from byolo import _lib, synth
    m = build_model(VARIANT, 608, 608, T=1)[1]
    eng = m.engine
    eng.set_params(synth.base_params(eng.param_shapes(), VARIANT, 2, seed=7))
    eng.finalize()
    cap = eng.max_images(1)
    B = cap + 1
    x = torch.from_numpy(synth.synthetic_images(2, 608, 608, seed=1234)).cuda()
    eng.calibrate_bn(x)
    x = x.repeat((B + 1) // 2, 1, 1, 1)[:B].contiguous()
    eng.forward(x, T=1, want_boxes=False, want_nms=True)
    N, D = eng.num_boxes()
    out = torch.full((1, 1, N, D), SENT, device="cuda")                   # (nothing may be written: one image's worth is enough)
    rc, msg = _ladder_rc(eng, B, 1, [1], out)
    torch.cuda.synchronize()
    assert rc == _lib.ERR_ARG and "pieces" in msg and (out == SENT).all(), msg
    with pytest.raises(_lib.ByoloError):
        eng.t_ladder([1], B, 1, out=torch.empty((1, B, N, D), device="cuda"))
    eng.close()


# ---- end to end, tiny ---------------------------------------------------------------------------------------------------------------
def test_evaluate_end_to_end(tmp_path):
    import evaluate
    from lib_yolo import yolov3
    from test_eval_gpu import BATCH, FRAMES, H, W, _pngs, _shards
    g = np.random.default_rng(3)
    gt = []
    for _ in range(FRAMES):                                               # a few boxes per frame: what is scored does not matter here
        y0, x0 = g.uniform(0.05, 0.5, 3), g.uniform(0.05, 0.5, 3)
        boxes = np.stack([y0, x0, y0 + g.uniform(0.2, 0.4, 3), x0 + g.uniform(0.1, 0.3, 3)], 1).astype(np.float32)
        gt.append((boxes, g.integers(0, 2, 3).astype(np.int64)))
    cfg = {'full_img_size': [H, W, 3], 'cls_cnt': 2, 'batch_size': BATCH, 'crop': False, 'priors': yolov3.ECP_9_PRIORS, 'T': 4,
           'implicit_background_class': True, 'weights': 'synthetic', 'seed': 5, 'cpu_thread_cnt': 2, 'eval_batches': 2,
           'iou_thresholds': [0.5, 0.75], 'data': {'file_pattern': _shards(str(tmp_path / 'shards'), _pngs(), gt)}}
    both = evaluate.evaluate(dict(cfg, out_path=str(tmp_path / 'both'), t_ladder=[1, 2]), 'bayesian')
    on_disk = json.load(open(str(tmp_path / 'both_0' / 'metrics.json')))
    assert on_disk['config']['t_ladder'] == [1, 2] and on_disk['images'] == 2 * BATCH
    main = [k for k in on_disk if k not in ('images', 'checkpoint', 'model', 'loop_seconds', 'steady_img_s', 'config', 't_ladder')]
    assert 'classes' in main and 'ladder' in main and 'localisation' in main and 'uncertainty' in main
    assert [e['T'] for e in on_disk['t_ladder']] == [1, 2]
    for e in on_disk['t_ladder']:
        assert sorted(k for k in e if k != 'T') == sorted(main)
    assert json.dumps(both['t_ladder']) == json.dumps(on_disk['t_ladder'])
    strip = lambda e: json.dumps({k: e[k] for k in main}, sort_keys=True)
    assert len({strip(on_disk['t_ladder'][0]), strip(on_disk['t_ladder'][1]), strip(on_disk)}) == 3, "three sample counts, three tables"
    alone = evaluate.evaluate(dict(cfg, out_path=str(tmp_path / 'alone'), t_ladder=[2]), 'bayesian')
    assert len(alone['t_ladder']) == 1
    assert json.dumps(alone['t_ladder'][0], sort_keys=True) == json.dumps(both['t_ladder'][1], sort_keys=True), "the rungs do not influence each other"
    assert strip(alone) == strip(both), "nor the full-T table"
    plain = evaluate.evaluate(dict(cfg, out_path=str(tmp_path / 'plain')), 'bayesian')
    assert 't_ladder' not in plain and 't_ladder' not in plain['config'] and strip(plain) == strip(both)
