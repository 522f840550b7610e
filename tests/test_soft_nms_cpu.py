"""Soft-NMS without a GPU: the numpy restatement (tests/_soft_nms_ref.py) against the pinned hard NMS in the setting where the two
coincide, its ordering rules, the condition under which tests/test_soft_nms_gpu.py may compare exactly, and the host side --
evaluate.check_config's new keys, Engine._soft_cfg's validation, the ctypes view of byolo_soft_nms_cfg."""
import ctypes
import os
import re

import numpy as np
import pytest

import _box_vote_ref as bv
import _nms_per_class_ref as pcr
import _soft_nms_ref as sr
from _soft_nms_ref import OBJ_IDX, CLS_START
from conftest import REPO
from oracle import nms_ref

F32 = np.float32


@pytest.mark.parametrize("boxes", ["spread", "clustered"])
def test_degenerate_setting_equals_the_hard_nms(boxes):
    """linear, iou_soft = 1, iou_hard = t, min_score = 0: every weight is 1 and a candidate leaves when its IoU with a pick exceeds t
    -- oracle.nms_ref.nms_tf over the candidates with score > 0, per class."""
    rows = pcr.random_rows(np.random.default_rng([21, len(boxes)]), 2, 3001, 3, boxes=boxes)
    assert (rows[..., OBJ_IDX] == 0).any()                   # scores of exactly 0 exist: the hard NMS takes them, min_score = 0 does not
    for mode, t in ((0, 0.5), (1, 0.5), (2, 0.3)):
        C = bv.n_classes(mode, 3)
        got = sr.soft_nms(rows, OBJ_IDX, CLS_START, mode, 3, 1000, method='linear', iou_soft=1.0, iou_hard=t, min_score=0.0)
        for b in range(2):
            cl = bv.row_classes(rows[b], OBJ_IDX, CLS_START, C)
            keeps = [nms_ref.nms_tf(rows[b][:, :4], rows[b][:, OBJ_IDX], 1000, t, candidates=(cl == c) & (rows[b][:, OBJ_IDX] > 0)) for c in range(C)]
            keep = np.concatenate(keeps)
            assert len(keep) > 30 and got['count'][b].tolist() == [len(keep), len(keeps[0])]
            assert np.array_equal(got['kept'][b, :len(keep)], keep), (mode, b)
            assert np.array_equal(got['rows'][b, :len(keep)].view(np.uint32), rows[b][keep].view(np.uint32))      # undecayed scores
            assert got['class_counts'][b].tolist() == [len(k) for k in keeps]


def test_ordering():
    """Output scores are non-increasing per class; exact duplicates of a row come out lower index first."""
    rows = sr.generator_rows(0, 2, 'clustered', B=1)
    for method in ('linear', 'gaussian'):
        ref = sr.soft_nms(rows, OBJ_IDX, CLS_START, 2, 3, 1000, method=method)
        lo = 0
        for n in ref['class_counts'][0]:
            s = ref['rows'][0, lo:lo + n, OBJ_IDX]
            assert n > 10 and (s[1:] <= s[:-1]).all() and (s[1:] < s[:-1]).any()
            lo += n
    # four far-apart boxes, each three times: a copy is picked behind the original, at the decayed score, lower index first
    one = np.zeros((12, pcr.row_len(2)), dtype=F32)
    for k in range(4):
        one[k::4, :4] = (k, k, k + 0.5, k + 0.5)
        one[k::4, OBJ_IDX] = 0.9 - 0.1 * k
    k, s = sr.soft_nms_class(one, OBJ_IDX, np.ones(12, bool), 1000, method='linear', min_score=0.0)
    assert k.tolist()[:4] == [0, 1, 2, 3] and s[:4].tolist() == [F32(0.9), F32(0.8), F32(0.7), F32(0.6)]
    assert len(k) == 4 and set(k.tolist()) == {0, 1, 2, 3}   # linear, IoU 1: the copies' weight is 0, they leave
    k, s = sr.soft_nms_class(one, OBJ_IDX, np.ones(12, bool), 1000, method='gaussian', sigma=0.5, min_score=0.0)
    w = F32(np.exp(-1.0 / np.float64(F32(0.5))))
    assert k.tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11]
    assert s[4] == F32(0.9) * w and s[8] == F32(F32(0.9) * w) * w and (s[1:] <= s[:-1]).all()
    k, _ = sr.soft_nms_class(one, OBJ_IDX, np.ones(12, bool), 1000, method='gaussian', iou_hard=0.7, min_score=0.0)
    assert k.tolist() == [0, 1, 2, 3]                        # removal outright: IoU 1 > iou_hard


@pytest.mark.parametrize("name", sorted(sr.cases()))
def test_seed_condition_for_the_gpu_cases(name):
    """Every input tests/test_soft_nms_gpu.py compares exactly: with every weight < 1 moved by one float32 ulp, up or down at random,
    three draws, the kept sequence is the same.  A float64 exp() of the device can differ from numpy's by an ulp of float64, which
    moves the float32 weight by one ulp at most and only on a rounding boundary -- far less than this."""
    (rows, mode, C, max_out, settings), ref = sr.reference(name)
    for draw in range(3):
        moved = sr.soft_nms(rows, OBJ_IDX, CLS_START, mode, C, max_out, perturb=sr.one_ulp(np.random.default_rng([5, draw])), **settings)
        assert np.array_equal(moved['kept'], ref['kept']) and np.array_equal(moved['count'], ref['count']), (name, draw)
    if 'mode' in name:                                       # the scores did move: the perturbation is not a no-op
        assert not np.array_equal(moved['rows'].view(np.uint32), ref['rows'].view(np.uint32))


def test_generator_cases_end_both_ways():
    """Clustered rows end by exhaustion, spread rows at max_out (the large class), for both methods."""
    for method in ('linear', 'gaussian'):
        _, a = sr.reference('%s-mode0-clustered' % method)
        _, b = sr.reference('%s-mode0-spread' % method)
        assert (a['class_counts'] < 1000).all() and (a['class_counts'] > 100).all() and (b['class_counts'] == 1000).all()


BASE = {'full_img_size': [64, 96, 3], 'cls_cnt': 2, 'batch_size': 2, 'crop': False, 'priors': None, 'implicit_background_class': True,
        'data': {'file_pattern': 'x-*'}, 'out_path': 'out', 'weights': 'synthetic'}


def test_check_config_keys():
    import evaluate
    plain = evaluate.check_config(dict(BASE))
    assert 'soft_nms' not in plain and 'soft_nms_compare' not in plain and 'soft_nms' not in plain.get('engine_options', {})
    on = evaluate.check_config(dict(BASE, soft_nms=True))
    assert on['soft_nms'] is True and on['soft_nms_compare'] is False and on['engine_options']['soft_nms'] is True
    st = {'method': 'linear', 'iou_soft': 0.4}
    on = evaluate.check_config(dict(BASE, soft_nms=st, engine_options={'nms_mode': 1}))
    assert on['engine_options'] == {'nms_mode': 1, 'soft_nms': st}
    cmp_ = evaluate.check_config(dict(BASE, soft_nms_compare=True))
    assert cmp_['soft_nms'] is True and cmp_['soft_nms_compare'] is True and 'soft_nms' not in cmp_.get('engine_options', {})
    cmp_ = evaluate.check_config(dict(BASE, soft_nms=st, soft_nms_compare=True))
    assert cmp_['soft_nms'] == st and 'engine_options' not in cmp_
    off = evaluate.check_config(dict(BASE, soft_nms=False))
    assert 'soft_nms' not in off.get('engine_options', {})
    with pytest.raises(ValueError, match='box_vote_compare'):
        evaluate.check_config(dict(BASE, soft_nms_compare=True, box_vote=True, box_vote_compare=True))
    with pytest.raises(ValueError, match='True or a dict'):
        evaluate.check_config(dict(BASE, soft_nms='gaussian'))
    with pytest.raises(ValueError, match='sigma'):
        evaluate.check_config(dict(BASE, soft_nms={'sigma': 0.0}))
    with pytest.raises(ValueError, match='unknown settings'):
        evaluate.check_config(dict(BASE, soft_nms={'sigma_t': 0.1}))
    with pytest.raises(ValueError, match='soft_nms_compare'):
        evaluate.check_config(dict(BASE, soft_nms_compare='yes'))


def test_settings_validation():
    from byolo import Engine, _lib
    c = Engine._soft_cfg({})
    assert (c.method, c.sigma, c.iou_soft, c.iou_hard, c.min_score) == (_lib.SOFT_NMS_GAUSSIAN, 0.5, F32(0.3), 1.0, F32(0.001))
    assert c.struct_bytes == ctypes.sizeof(_lib.SoftNmsCfg) == 24
    assert {k: v for k, v in Engine.SOFT_DEFAULTS.items()} == sr.DEFAULTS
    assert Engine._soft_cfg({'method': 'linear'}).method == _lib.SOFT_NMS_LINEAR
    for bad, field in (({'method': 'quadratic'}, 'method'), ({'sigma': 0}, 'sigma'), ({'sigma': -1.0}, 'sigma'), ({'sigma': float('nan')}, 'sigma'),
                       ({'sigma': float('inf')}, 'sigma'), ({'iou_soft': -0.1}, 'iou_soft'), ({'iou_soft': 1.5}, 'iou_soft'),
                       ({'iou_hard': float('nan')}, 'iou_hard'), ({'iou_hard': 2}, 'iou_hard'), ({'min_score': -1e-3}, 'min_score'),
                       ({'min_score': float('inf')}, 'min_score'), ({'min_score': None}, 'min_score'), ({'sigma': '0.5'}, 'sigma')):
        with pytest.raises(ValueError, match=field):
            Engine._soft_cfg(bad)
    with pytest.raises(TypeError, match='iou_thresh'):
        Engine._soft_cfg({'iou_thresh': 0.5})


def test_the_library_refuses_bad_settings_by_name():
    """byolo_set_soft_nms validates before anything touches a device: BYOLO_ERR_ARG with the field in the message."""
    from byolo import _lib
    h = ctypes.c_void_p()
    cfg = _lib.Cfg(64, 96, 3, 2, 0.1, 1000, 0.5, 0, 0)
    assert _lib.lib.byolo_create(ctypes.byref(cfg), 0, ctypes.byref(h)) == 0
    good = dict(struct_bytes=ctypes.sizeof(_lib.SoftNmsCfg), method=1, sigma=0.5, iou_soft=0.3, iou_hard=1.0, min_score=0.001)
    assert _lib.lib.byolo_set_soft_nms(h, ctypes.byref(_lib.SoftNmsCfg(**good))) == 0
    assert _lib.lib.byolo_set_soft_nms(h, None) == 0
    for field, value in (('struct_bytes', 20), ('method', 2), ('sigma', 0.0), ('sigma', float('nan')), ('iou_soft', 1.5), ('iou_hard', -0.5),
                         ('min_score', -1.0), ('min_score', float('inf'))):
        c = _lib.SoftNmsCfg(**dict(good, **{field: value}))
        assert _lib.lib.byolo_set_soft_nms(h, ctypes.byref(c)) == _lib.ERR_ARG
        assert field.encode() in _lib.lib.byolo_last_error(h), (field, _lib.lib.byolo_last_error(h))
    assert _lib.lib.byolo_soft_nms_workspace_bytes(2, 3001, 0, 2) > 0
    assert _lib.lib.byolo_soft_nms_workspace_bytes(2, 3001, 2, 3) > _lib.lib.byolo_soft_nms_workspace_bytes(2, 3001, 1, 3)
    assert _lib.lib.byolo_soft_nms_workspace_bytes(2, 3001, 3, 2) == 0 and _lib.lib.byolo_soft_nms_workspace_bytes(0, 3001, 0, 2) == 0
    assert _lib.lib.byolo_nms_workspace_bytes(8, 22743) == _lib.lib.byolo_nms_workspace_bytes_ex(8, 22743, 1, 2)      # untouched
    _lib.lib.byolo_destroy(h)


def test_cfg_struct_and_capacity_match_the_header():
    from byolo import _lib
    text = open(os.path.join(REPO, "include", "byolo.h")).read()
    body = re.search(r"typedef struct byolo_soft_nms_cfg \{(.*?)\} byolo_soft_nms_cfg;", text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        if decl.strip():
            ty, names = decl.strip().split(None, 1)
            fields += [(n.strip(), {"int32_t": ctypes.c_int32, "float": ctypes.c_float}[ty]) for n in names.split(",")]
    assert fields == list(_lib.SoftNmsCfg._fields_)
    assert int(re.search(r"#define BYOLO_SOFT_NMS_RESIDENT (\d+)", text).group(1)) == _lib.SOFT_NMS_RESIDENT == sr.RESIDENT
    assert re.search(r"BYOLO_SOFT_NMS_LINEAR = (\d), BYOLO_SOFT_NMS_GAUSSIAN = (\d)", text).groups() == (str(_lib.SOFT_NMS_LINEAR), str(_lib.SOFT_NMS_GAUSSIAN))
    assert re.search(r"#define BYOLO_ABI_VERSION\s+(\d+)", text) is None or int(re.search(r"#define BYOLO_ABI_VERSION\s+(\d+)", text).group(1)) == _lib.ABI_VERSION
