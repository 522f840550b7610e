"""A batch beyond byolo_max_images(T) with every stage behind the decode switched on: byolo_forward runs it as consecutive pieces in
one workspace and copies each piece's per-image side outputs (class counts, vote counts, calibrated scores) out behind it.  The
whole-batch call is compared bit for bit with the two calls that have the pieces' batch sizes and positions."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

VARIANT, CLS, H, W = "yolov3_aleatoric", 3, 608, 608
KEYS = ("boxes", "rows", "kept", "count", "class_counts", "vote_n", "score")


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


@pytest.fixture(scope="module")
def model():
    from conftest import build_model
    from byolo import synth
    m = build_model(VARIANT, H, W, T=1, cls_cnt=CLS, engine_options={"nms_mode": 2})[1]
    eng = m.engine
    eng.set_params(synth.base_params(eng.param_shapes(), VARIANT, CLS, seed=7))
    eng.finalize()
    cap = eng.max_images(1)
    B = cap + 1
    x = torch.from_numpy(synth.synthetic_images(B, H, W, seed=1234)).cuda()
    eng.calibrate_bn(x[:2])
    yield m, x, cap, B
    eng.close()


@pytest.mark.parametrize("soft", [False, True], ids=["hard", "soft"])
def test_pieces_with_votes_and_scores_equal_their_own_calls(model, soft):
    from byolo import _lib
    from byolo.score_recal import ScoreCalibration
    m, x, cap, B = model
    eng = m.engine
    assert 1 <= cap < B, "the batch must exceed one call's capacity (%d) for this test to mean anything" % cap
    rng = np.random.default_rng(23)
    cal = ScoreCalibration(VARIANT, CLS, None, "class")
    for g in range(cal.n_groups):
        cal.w[g] = [float(rng.normal(0.0, 0.5)), float(rng.uniform(0.5, 1.5))] + [float(v) for v in rng.normal(0.0, 0.2, cal.K - 2)]
    eng.set_soft_nms(True if soft else None)
    eng.set_box_vote(True)
    try:
        eng.set_score_recal(ScoreCalibration(VARIANT, CLS, None, "class"))       # the identity: score is bitwise obj * cls[c]
        plain = eng.forward(x[:2], T=1, want_boxes=True, want_nms=True)["score"]
        eng.set_score_recal(cal)
        first = eng.forward(x[:cap], T=1, want_boxes=True, want_nms=True, first_image=0)
        second = eng.forward(x[cap:], T=1, want_boxes=True, want_nms=True, first_image=cap)
        whole = eng.forward(x, T=1, want_boxes=True, want_nms=True)
        torch.cuda.synchronize()
        assert set(KEYS) <= set(whole), sorted(whole)
        for k in KEYS:
            assert whole[k].shape[0] == B and first[k].shape[0] == cap and second[k].shape[0] == B - cap, k
            assert torch.equal(_bits(whole[k][:cap]), _bits(first[k])), (soft, k, "first piece")
            assert torch.equal(_bits(whole[k][cap:]), _bits(second[k])), (soft, k, "second piece")
        # the getters answer for the whole batch, and for nothing else
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        out_cap = eng.out_cap
        for fn, cols, dtype, key in ((_lib.lib.byolo_nms_class_counts, CLS, torch.int32, "class_counts"),
                                     (_lib.lib.byolo_box_vote_counts, out_cap, torch.int32, "vote_n"),
                                     (_lib.lib.byolo_score_recal_scores, out_cap, torch.float32, "score")):
            buf = torch.zeros((B, cols), dtype=dtype, device=x.device)
            assert fn(eng._h, ctypes.c_void_p(buf.data_ptr()), B, cols, stream) == 0, key
            torch.cuda.synchronize()
            assert torch.equal(_bits(buf), _bits(whole[key])), key
            assert fn(eng._h, ctypes.c_void_p(buf.data_ptr()), cap, cols, stream) == _lib.ERR_ARG, key
        # what keeps all of the above from passing on nothing
        count = whole["count"][:, 0]
        assert all(int(count[i]) > 0 for i in (0, cap - 1, cap)), count[[0, cap - 1, cap]].tolist()
        assert torch.equal(whole["class_counts"].sum(1, dtype=torch.int32), count)
        assert int(whole["vote_n"].max()) > 1
        assert not torch.equal(_bits(whole["score"][:2]), _bits(plain))
    finally:
        eng.set_score_recal(None)
        eng.set_box_vote(None)
        eng.set_soft_nms(None)
