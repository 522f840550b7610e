"""The planner's lowering of a STEP_REP / STEP_FINISH step INTO the Winograd input transform of the convolution that alone reads it
(byolo_plan_opts.wino_split_feed, csrc/byolo_plan.hip Plan::feed) -- on the CPU, through byolo_plan_*:

  * the tensor in between has no arena range, the producer's operands (the per-image raw accumulators; the low-resolution sums and the
    per-image partial sums) stay alive until the reader, and THE INVARIANT of tests/test_planner.py holds: no tensor is written
    while another that shares its memory is alive -- reference models, hand-built heads, random graphs, every value of the option;
  * a producer whose output has a second reader, an fp32 handle, a reader that stays on the direct kernel and keep_all_outputs keep
    the two-launch plan.

How a folded step shows in the introspection: a folded STEP_REP reports the auxiliary raw-accumulator tensor as its output, a folded
STEP_FINISH (no launch) reports the `low` operand it hands on, and the reader reports those operands as what it reads.
The reference has no counterpart (TensorFlow owns its tensors)."""
import numpy as np
import pytest

from conftest import build_model
from test_planner import KNOBS, _plan, _random_graph, check_plan

PRIORS = [(0.1, 0.2), (0.3, 0.1), (0.5, 0.5)]
FEED_KNOBS = dict(KNOBS, BYOLO_WINO_SPLIT_FEED=("0", "1", "2", "3"))


def _clear(monkeypatch):
    for k in list(FEED_KNOBS) + ["BYOLO_PRECISION", "BYOLO_WINO_SPLIT_MIN_C", "BYOLO_WINO_SPLIT_MIN_GFLOP"]:
        monkeypatch.delenv(k, raising=False)


def _folded(plan_off, plan_on, n_layers=None):
    """Tensors that have memory in the two-launch plan and none with the option on."""
    return [t for t, (a, b) in enumerate(zip(plan_off[1], plan_on[1])) if a[0] >= 0 and b[0] < 0]


def _head(second_reader=None, keep_all=False, hw=(64, 96), c=128):
    """A two-scale Bayesian head in the reference's shape (lib_yolo/yolov3.py:518-628) at the smallest channel counts the split
    Winograd kernel takes: layer 4 = the 1x1 dropout convolution over the T-fold tile (STEP_REP), read by the 3x3 convolution 5;
    layer 13 = the 1x1 concat convolution over [upsampled, stacked skip] (STEP_PARTIAL x 2 + STEP_FINISH), read by the 3x3
    convolution 14.  second_reader = 4 | 13: one more head reads that layer's output through a route."""
    from byolo import Engine
    eng = Engine((hw[0], hw[1], 3), 2, keep_all_outputs=keep_all)
    eng.add_conv("c0", 32, 3, 1, 1)           # 0   64 x 96
    eng.add_conv("c1", c, 3, 2, 1)            # 1   32 x 48: the skip
    eng.add_conv("c2", c, 3, 2, 1)            # 2   16 x 24
    eng.add_stack(2)                          # 3
    eng.add_conv("h0", c, 1, 1, 3)            # 4   STEP_REP
    eng.add_conv("h1", 2 * c, 3, 1, 3)        # 5   its reader
    eng.add_conv("h2", c, 1, 1, 3)            # 6
    eng.add_detection("d0/detection", 2, PRIORS)   # 7
    eng.add_route([6])                        # 8
    eng.add_conv("h3", c, 1, 1, 1)            # 9
    eng.add_upsample()                        # 10
    eng.add_stack(1)                          # 11
    eng.add_route([10, 11])                   # 12
    eng.add_conv("h4", c, 1, 1, 3)            # 13  STEP_PARTIAL, STEP_PARTIAL (low), STEP_FINISH
    eng.add_conv("h5", 2 * c, 3, 1, 3)        # 14  its reader
    eng.add_detection("d1/detection", 2, PRIORS)   # 15
    if second_reader is not None:
        eng.add_route([second_reader])
        eng.add_conv("x0", 128, 1, 1, 1)
        eng.add_detection("d2/detection", 2, PRIORS)
    return eng


@pytest.mark.parametrize("H,W,B,T", [(608, 608, 8, 30), (1024, 1920, 1, 50)])
def test_reference_bayesian_plan_folds_the_two_intermediate_tensors(H, W, B, T, monkeypatch):
    """The benchmark's plans: with the option on (the default) exactly the two tensors between an element-wise pass and a Winograd
    transform -- the outputs of the 19x19 head's first 1x1 convolution and of the 38x38 head's concat convolution -- have no arena
    range and the plan keeps live tensors apart (the arena's size is the first-fit layout's, set by the 76x76 head: not asserted); bit 0 / bit 1 alone fold one of them each."""
    _clear(monkeypatch)
    _, m = build_model("bayesian_yolov3_aleatoric", H, W, T=T)
    assert m.engine.plan_opts()["wino_split_feed"] == 3
    plans = {}
    for feed in (0, 1, 2, 3):
        m.engine.set_plan_opts(wino_split_feed=feed)
        for inject in (0, 1):
            plans[feed, inject] = _plan(m.engine, B, T, inject)
            check_plan(*plans[feed, inject], "bayesian %dx%d B=%d T=%d feed=%d inject=%d" % (H, W, B, T, feed, inject))
    for inject in (0, 1):
        off, on = plans[0, inject], plans[3, inject]
        gone = _folded(off, on)
        assert len(gone) == 2, gone
        sizes = sorted(off[1][t][1] for t in gone)
        S = B * T
        assert sizes == sorted([S * (H // 32) * (W // 32) * 512 * 4, S * (H // 16) * (W // 16) * 256 * 4])
        one, two = _folded(off, plans[1, inject]), _folded(off, plans[2, inject])
        assert len(one) == 1 and len(two) == 1 and sorted(one + two) == sorted(gone)
        assert off[1][one[0]][1] == sizes[0] and off[1][two[0]][1] == sizes[1]
        # the folded tensors are named by no step of the plan any more, and no other tensor lost its memory
        named = {s[0] for s in on[0]} | {t for s in on[0] for t in s[2]}
        assert not (named & set(gone))
        assert all((a[0] >= 0) == (b[0] >= 0) or t in gone or a[0] < 0 for t, (a, b) in enumerate(zip(off[1], on[1])))
    m.engine.close()


def test_other_models_and_modes_keep_their_plans(monkeypatch):
    """Nothing to fold in the fp32 mode, in the models without T-stacking, with the Winograd layers off, or where the time model keeps
    the readers on the direct kernel (64 x 96): the plan is the two-launch plan, tensor for tensor."""
    _clear(monkeypatch)
    cases = [("bayesian_yolov3_aleatoric", 608, 608, 8, 30, {"BYOLO_PRECISION": "f32"}), ("bayesian_yolov3_aleatoric", 608, 608, 8, 30, {"BYOLO_WINO_SPLIT": "0"}),
             ("bayesian_yolov3_aleatoric", 64, 96, 2, 3, {}), ("yolov3_aleatoric", 416, 416, 8, 1, {}), ("yolov3", 416, 416, 1, 1, {})]
    for variant, H, W, B, T, env in cases:
        _clear(monkeypatch)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        _, m = build_model(variant, H, W, T=T)
        on = _plan(m.engine, B, T)
        m.engine.set_plan_opts(wino_split_feed=0)
        assert _plan(m.engine, B, T) == on, (variant, env)
        m.engine.close()


def test_small_head_folds_when_every_layer_is_transformed(monkeypatch):
    """The hand-built head (and the reference model at 64 x 96, the GPU test's size) with wino_split = 2: layers 4 and 13 are folded,
    their readers read the producers' operands, and the option is a [plan] field -- no re-pack."""
    _clear(monkeypatch)
    eng = _head()
    eng.set_plan_opts(wino_split=2, wino_split_min_c=128, wino_split_min_gflop=0.0)
    for B, T in ((1, 2), (2, 3), (3, 1)):
        on = _plan(eng, B, T)
        check_plan(*on, "head B=%d T=%d" % (B, T))
        eng.set_plan_opts(wino_split_feed=0)
        off = _plan(eng, B, T)
        check_plan(*off, "head B=%d T=%d, two launches" % (B, T))
        eng.set_plan_opts(wino_split_feed=3)
        assert _folded(off, on) == [4, 13]
        # the readers: same step index in both plans; what they read changed from the folded tensor to auxiliary tensors (ids >= 16)
        for t in (4, 13):
            ri = next(i for i, s in enumerate(off[0]) if t in s[2])
            assert on[0][ri][0] == off[0][ri][0] and all(x >= 16 for x in on[0][ri][2]) and len(on[0][ri][2]) == (1 if t == 4 else 2)
    eng.close()
    _, m = build_model("bayesian_yolov3_aleatoric", 64, 96, T=3)
    m.engine.set_plan_opts(wino_split=2, wino_split_min_c=128, wino_split_min_gflop=0.0)
    on = _plan(m.engine, 2, 3)
    m.engine.set_plan_opts(wino_split_feed=0)
    # (layers 76 and 88 as at the benchmark's size; with every layer transformed the 76x76 head's concat convolution 100 follows the same rule)
    assert _folded(_plan(m.engine, 2, 3), on) == [76, 88, 100]
    m.engine.close()


@pytest.mark.parametrize("second", [4, 13])
def test_a_second_reader_keeps_the_two_launch_lowering(second, monkeypatch):
    """One more head reads the STEP_REP's (4) or the STEP_FINISH's (13) output through a route: that tensor must exist, so only the
    other producer is folded; keep_all_outputs (every tensor is read after the steps) folds none."""
    _clear(monkeypatch)
    eng = _head(second_reader=second)
    eng.set_plan_opts(wino_split=2, wino_split_min_c=128, wino_split_min_gflop=0.0)
    on = _plan(eng, 2, 3)
    check_plan(*on, "head with a second reader of %d" % second)
    eng.set_plan_opts(wino_split_feed=0)
    off = _plan(eng, 2, 3)
    assert _folded(off, on) == [13 if second == 4 else 4]
    assert on[1][second][0] >= 0
    eng.close()
    eng = _head(keep_all=True)
    eng.set_plan_opts(wino_split=2, wino_split_min_c=128, wino_split_min_gflop=0.0)
    on = _plan(eng, 2, 3)
    check_plan(*on, "head, keep_all_outputs")
    eng.set_plan_opts(wino_split_feed=0)
    assert _plan(eng, 2, 3) == on
    eng.close()


def test_random_graphs_with_the_option_never_alias_a_live_tensor(monkeypatch):
    """The random graphs of tests/test_planner.py (same generator), split-f16, every planning knob at random INCLUDING the feed
    option and with wino_split = 2 half of the time so that small layers are transformed, every third graph a two-scale Bayesian head
    (the generator's graphs hardly ever put a foldable step in front of a transformed layer): the invariant holds, and steps were folded."""
    from byolo import ByoloError
    _clear(monkeypatch)
    monkeypatch.setenv("BYOLO_PRECISION", "split")
    monkeypatch.setenv("BYOLO_WINO_SPLIT_MIN_C", "128")
    rng = np.random.default_rng(20261016)
    done = refused = folded = pairs = 0
    while done < 300:
        for k, vals in FEED_KNOBS.items():
            v = str(rng.choice(("",) + vals))
            if k == "BYOLO_WINO_SPLIT" and rng.random() < 0.5:
                v = "2"
            if v:
                monkeypatch.setenv(k, v)
            else:
                monkeypatch.delenv(k, raising=False)
        try:
            if done % 3 == 2:                                # every third graph: the head above at a random size, with or without second readers
                T = int(rng.integers(1, 5))
                if rng.random() < 0.8:
                    monkeypatch.setenv("BYOLO_WINO_SPLIT", "2")
                eng = _head(second_reader=[None, 4, 13][int(rng.integers(0, 3))], keep_all=bool(rng.random() < 0.1),
                            hw=(int(rng.integers(1, 4)) * 64, int(rng.integers(1, 4)) * 64), c=int(rng.choice([128, 256])))
            else:
                eng, T = _random_graph(rng)
        except ByoloError:
            refused += 1
            continue
        B = int(rng.integers(1, 5))
        try:
            for inject in (0, 1):
                steps, tensors, arena = _plan(eng, B, T, inject)
                _, b = check_plan(steps, tensors, arena, "random graph %d B=%d T=%d inject=%d" % (done, B, T, inject))
                pairs += b
                feed = eng.plan_opts()["wino_split_feed"]
                if feed:
                    eng.set_plan_opts(wino_split_feed=0)
                    folded += len(_folded(_plan(eng, B, T, inject), (steps, tensors, arena)))
                    eng.set_plan_opts(wino_split_feed=feed)
            done += 1
        except ByoloError:
            refused += 1
        finally:
            eng.close()
    print("%d graphs planned (%d refused), %d memory-sharing tensor pairs checked, %d steps folded" % (done, refused, pairs, folded))
    assert pairs > 1000 and refused < 3 * done and folded > 30, "too few folded steps for the invariant to have been checked on them"
