"""The MC sample-count ladder without a GPU: the `t_ladder` key of evaluate.check_config, and the ABI's additions (two prototypes,
BYOLO_T_LADDER_MAX in the header and in the binding, the ABI version unchanged)."""
import os
import re

import pytest

from conftest import REPO


def _cfg(**kw):
    from lib_yolo import yolov3
    c = {'full_img_size': [64, 96, 3], 'cls_cnt': 2, 'batch_size': 3, 'crop': False, 'priors': yolov3.ECP_9_PRIORS, 'T': 30,
         'implicit_background_class': True, 'weights': 'synthetic', 'out_path': '/nowhere/run', 'data': {'file_pattern': '/nowhere/*'}}
    c.update(kw)
    return c


def test_check_config_accepts_and_normalises():
    import evaluate
    import numpy as np
    got = evaluate.check_config(_cfg(t_ladder=(5, np.int64(10), 20)), 'bayesian')
    assert got['t_ladder'] == [5, 10, 20] and all(type(r) is int for r in got['t_ladder'])
    assert evaluate.check_config(_cfg(t_ladder=[29]), 'bayesian')['t_ladder'] == [29]
    assert evaluate.check_config(_cfg(t_ladder=list(range(1, 9))), 'bayesian')['t_ladder'] == list(range(1, 9))
    assert 't_ladder' not in evaluate.check_config(_cfg(), 'bayesian')            # absent stays absent: metrics.json carries the config
    # the stages of the model's own tail go along (each rung passes through them), the IoU ladder and the subsets too
    evaluate.check_config(_cfg(t_ladder=[5], box_vote=True, soft_nms=True, iou_thresholds='coco', eval_subsets='ecp_heights'), 'bayesian')


@pytest.mark.parametrize("bad", [5, '5,10', {5: 1}, [], list(range(1, 10)), [10, 5], [5, 5], [0, 5], [-1], [5, 30], [31], [2.5], [True],
                                 ['5'], [None]], ids=repr)
def test_check_config_refuses_bad_rungs(bad):
    import evaluate
    with pytest.raises(ValueError, match='t_ladder'):
        evaluate.check_config(_cfg(t_ladder=bad), 'bayesian')


def test_check_config_refuses_T_of_one_and_other_models():
    import evaluate
    c = _cfg(t_ladder=[1])
    del c['T']                                                                   # T defaults to 1: no rung lies below it
    with pytest.raises(ValueError, match='t_ladder: every rung lies below T = 1'):
        evaluate.check_config(c, 'bayesian')
    for model in ('standard', 'aleatoric'):
        with pytest.raises(ValueError, match='t_ladder: only the bayesian model'):
            evaluate.check_config(_cfg(t_ladder=[5]), model)


@pytest.mark.parametrize("other", [dict(box_vote=True, box_vote_compare=True), dict(soft_nms_compare=True),
                                   dict(var_recal='/nowhere/cal.json', var_recal_compare=True),
                                   dict(score_recal='/nowhere/cal.json', score_recal_compare=True),
                                   dict(box_vote=True, box_vote_compare=True, box_vote_sweep=[{'sigma_t': 0.02}])],
                         ids=lambda o: '+'.join(sorted(o)))
def test_check_config_refuses_a_second_comparison(other):
    import evaluate
    evaluate.check_config(_cfg(**other), 'bayesian')                             # fine by itself
    with pytest.raises(ValueError, match='t_ladder together with .*one comparison per run') as e:
        evaluate.check_config(_cfg(t_ladder=[5, 10], **other), 'bayesian')
    for k in other:
        if k.endswith('_compare') or k == 'box_vote_sweep':
            assert k in str(e.value)


def test_the_abi_carries_the_ladder():
    import ctypes
    from byolo import _lib
    text = open(os.path.join(REPO, "include", "byolo.h")).read()
    assert int(re.search(r"#define BYOLO_T_LADDER_MAX (\d+)", text).group(1)) == _lib.T_LADDER_MAX == 16
    assert int(re.search(r"#define BYOLO_T_LADDER_MAX_CLASSES (\d+)", text).group(1)) == _lib.T_LADDER_MAX_CLASSES
    assert int(re.search(r"#define BYOLO_ABI_VERSION (\d+)", text).group(1)) == 7 == _lib.lib.byolo_abi_version()
    i32, i64, vp = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p
    P = ctypes.POINTER
    assert _lib.PROTOTYPES["byolo_decode_ladder"] == (i32, [vp, vp, i32, i32, i32, i32, P(ctypes.c_float), i32, P(i32), i32, vp, i64, i64, vp])
    assert _lib.PROTOTYPES["byolo_forward_ladder"] == (i32, [vp, i32, i32, P(i32), i32, vp, vp])
    for name in ("byolo_decode_ladder", "byolo_forward_ladder"):
        assert getattr(_lib.lib, name).argtypes == _lib.PROTOTYPES[name][1]
        assert re.search(r"BYOLO_API int32_t %s\(" % name, text)
    # refused without a handle, and without touching a device
    assert _lib.lib.byolo_forward_ladder(None, 1, 1, (i32 * 1)(1), 1, None, None) == _lib.ERR_ARG
    assert _lib.lib.byolo_decode_ladder(None, None, 1, 1, 1, 1, None, 0, (i32 * 1)(1), 1, None, 3, 0, None) == _lib.ERR_ARG
