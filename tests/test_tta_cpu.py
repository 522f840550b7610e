"""Test-time augmentation without a GPU: the numpy restatement (tests/_tta_ref.py) on hand cases, the settings, what the entry
points refuse before anything is launched, and the ctypes struct against the header."""
import ctypes
import os
import re

import numpy as np
import pytest

import _tta_ref as tr
from conftest import REPO

F32 = np.float32


def _row(box, score, cls=(), D=None):
    r = list(box) + [score] + list(cls)
    return r + [0.0] * ((D or len(r)) - len(r))


# ---- the reference on hand cases ------------------------------------------------------------------------------------------------
def test_merge_mirrors_columns_1_and_3_and_offsets_the_layer_id():
    rows = np.zeros((1, 3, 16), F32)                                     # aleatoric rows, C = 2: layer id in column 14
    rows[0, :, :4] = [[0.1, 0.2, 0.5, 0.6], [0.3, np.nan, 0.4, 0.25], [0.0, np.inf, 1.0, -0.5]]
    rows[0, :, 14] = [2.0, np.nan, np.inf]
    rows[0, :, 15] = [0.0, 1.0, 2.0]
    union, off = tr.merge([(rows, False, 0), (rows, True, 1)], layer_col=14)
    assert off.tolist() == [0, 3, 6] and union.shape == (1, 6, 16)
    assert tr.same_bits(union[:, :3], rows)                              # the identity view keeps every bit
    m = union[0, 3:]
    assert m[0, 1] == F32(1.0) - F32(0.6) and m[0, 3] == F32(1.0) - F32(0.2)
    assert np.isnan(m[1, 3]) and m[1, 1] == F32(0.75)                    # a NaN stays a NaN, in the column it moves to
    assert m[2, 1] == F32(1.5) and m[2, 3] == -np.inf
    assert tr.same_bits(m[:, [0, 2]], rows[0][:, [0, 2]]) and tr.same_bits(m[:, 4:14], rows[0][:, 4:14]) and tr.same_bits(m[:, 15], rows[0][:, 15])
    assert m[0, 14] == 5.0 and np.isnan(m[1, 14]) and np.isinf(m[2, 14])  # 2 + 3 * 1; non-finite ids keep their bits
    std, _ = tr.merge([(rows[..., :7], True, 1)], layer_col=-1)          # standard rows: no id column
    assert tr.same_bits(std[..., 4:], rows[..., 4:7])


def test_support_picks_the_best_witness_of_every_view():
    # agnostic rows (box, score): view 0 = rows 0 - 2, view 1 = rows 3 - 5, view 2 = rows 6 - 7
    union = np.array([
        _row([0.10, 0.10, 0.50, 0.50], 0.9),       # 0 kept
        _row([0.10, 0.10, 0.50, 0.52], 0.95),      # 1 overlaps row 0 with a higher score: view 0's witness
        _row([0.60, 0.60, 0.90, 0.90], 0.8),       # 2 kept, far away
        _row([0.10, 0.12, 0.50, 0.50], 0.7),       # 3 } a tie inside view 1: the lower index wins
        _row([0.10, 0.10, 0.50, 0.48], 0.7),       # 4 }
        _row([0.10, 0.10, 0.50, 0.50], np.nan),    # 5 a NaN score is no witness
        _row([0.10, 0.10, 0.50, 0.50], 0.0005),    # 6 below min_score
        _row([0.10, np.inf, 0.50, 0.50], 0.99),    # 7 a box value that is not finite
    ], F32)
    kept = np.array([0, 2, -1, -1], np.int32)
    n, bits, score, var, wit = tr.support_image(union, kept, 2, [0, 3, 6, 8], obj_idx=4, cls_start=5, C=1)
    assert wit[0].tolist() == [1, 3, -1] and wit[1].tolist() == [2, -1, -1]
    assert n.tolist() == [2, 1, 0, 0] and bits.tolist() == [3, 1, 0, 0]
    assert score[0] == F32((np.float64(F32(0.95)) + np.float64(F32(0.7))) / 3.0) and score[1] == F32(np.float64(F32(0.8)) / 3.0)
    cx = [(np.float64(F32(0.10)) + np.float64(F32(0.52))) * 0.5, (np.float64(F32(0.12)) + np.float64(F32(0.50))) * 0.5]
    mean = (cx[0] + cx[1]) / 2.0
    assert var[0, 0] == F32(((cx[0] - mean) ** 2 + (cx[1] - mean) ** 2) / 2.0) and var[0, 1] == 0 and var[0, 3] == 0
    assert (var[1:] == 0).all() and (score[2:] == 0).all()              # one witness: variance 0; padding: zeros
    n0 = tr.support_image(union, kept, 0, [0, 3, 6, 8], obj_idx=4, cls_start=5, C=1)[0]
    assert (n0 == 0).all()                                               # count = 0


def test_support_class_rules():
    # per-class rows (box, score, two class scores): a witness has the kept row's class; a class tie belongs to no class
    box = [0.1, 0.1, 0.5, 0.5]
    union = np.array([_row(box, 0.9, (0.8, 0.1)), _row(box, 0.5, (0.5, 0.5)), _row(box, 0.6, (0.1, 0.8)), _row(box, 0.4, (0.9, 0.2))], F32)
    n, bits, _, _, wit = tr.support_image(union, np.array([0, 1], np.int32), 2, [0, 2, 4], obj_idx=4, cls_start=5, C=2)
    assert wit[0].tolist() == [0, 3] and n[0] == 2
    assert wit[1].tolist() == [-1, -1] and n[1] == 0 and bits[1] == 0    # the kept row itself has no class
    zero = np.array([_row([0.3, 0.3, 0.3, 0.6], 0.9, (0.8, 0.1)), _row([0.3, 0.3, 0.3, 0.6], 0.9, (0.8, 0.1))], F32)
    assert tr.support_image(zero, np.array([0], np.int32), 1, [0, 1, 2], obj_idx=4, cls_start=5, C=2)[0][0] == 0      # zero area: IoU 0


def test_view_is_resize_then_flip():
    g = np.random.default_rng(3)
    f = (g.integers(0, 256, (2, 8, 12, 3)).astype(F32) * (F32(1) / F32(255))).astype(F32)
    assert tr.same_bits(tr.view_f32(f, True, 8, 12), f[:, :, ::-1])
    assert tr.same_bits(tr.view_f32(f, False, 8, 12), f)
    up = tr.view_f32(f, False, 16, 24)
    assert up.shape == (2, 16, 24, 3) and tr.same_bits(up[:, ::2, ::2], f)          # src = dst * in / out: even pixels are the source's
    assert tr.same_bits(tr.view_f32(f, True, 16, 24), up[:, :, ::-1])


# ---- settings ----------------------------------------------------------------------------------------------------------------------
def test_settings():
    from byolo import tta
    full = (64, 96)
    s = tta.check_settings(True, full)
    assert s['views'] == [{'flip': False, 'size': full}, {'flip': True, 'size': full}] and s['sizes'] == [full]
    assert s['iou_min'] == 0.5 and s['min_score'] == float(F32(0.001))
    assert tta.check_settings({'flip': False}, full)['views'] == [{'flip': False, 'size': full}]
    s = tta.check_settings({'flip': True, 'sizes': [[96, 128]], 'iou_min': 0.4}, full)
    assert [(v['flip'], v['size']) for v in s['views']] == [(False, full), (True, full), (False, (96, 128)), (True, (96, 128))]
    assert s['sizes'] == [full, (96, 128)] and s['iou_min'] == float(F32(0.4))
    s = tta.check_settings([{'flip': False, 'size': None}, {'flip': True, 'size': [96, 128]}], full)
    assert s['views'][1] == {'flip': True, 'size': (96, 128)}
    for bad, field in (({'flip': 1}, 'flip'), ({'sizes': [[100, 128]]}, 'sizes[0]'), ({'sizes': [[96, 128], [128, 160]]}, 'sizes'),
                       ({'sizes': [96, 128]}, 'sizes[0]'), ({'iou_min': -0.1}, 'iou_min'), ({'iou_min': 'x'}, 'iou_min'),
                       ({'min_score': float('nan')}, 'min_score'), ({'no_such': 1}, 'no_such'), ('yes', 'settings'),
                       ({'views': [{'flip': True, 'size': None}]}, 'views[0]'), ({'views': [{'flip': False}, {'size': [33, 64]}]}, 'views[1].size'),
                       ({'views': [{'flip': False}] + [{'flip': True}] * 8}, 'views'), ({'views': [{'flip': False}], 'flip': True}, 'views'),
                       ({'views': [{'flip': False}, {'size': [96, 128]}, {'size': [128, 160]}]}, 'sizes')):
        with pytest.raises(ValueError) as e:
            tta.check_settings(bad, full)
        assert field in str(e.value), (bad, str(e.value))
    assert tta.view_seed(5, 0) == 5 and tta.view_seed(2**64 - 1, 1) == (2**64 - 1 + 0x9E3779B97F4A7C15) % 2**64


def test_model_option_and_what_run_refuses():
    """engine_options={'tta': ...} is checked when the model is built (in all three classes: lib_yolo/model.py ModelBuilder); a T
    shard, injected masks and a run without the NMS are ValueErrors before anything reaches the device."""
    from conftest import build_model
    for variant in ('yolov3', 'yolov3_aleatoric', 'bayesian_yolov3_aleatoric'):
        m = build_model(variant, 64, 96, T=2, engine_options={'tta': True})[1]
        assert m.tta is not None and len(m.tta.views) == 2 and len(m.tta.geometry()) == 3
        m.engine.close()
    assert build_model('yolov3_aleatoric', 64, 96, T=1)[1].tta is None
    for bad, field in (({'sizes': [[96, 100]]}, 'sizes[0]'), ({'sizes': [[96, 128], [128, 128]]}, 'sizes'), ({'views': [{'flip': False}] * 9}, 'views')):
        with pytest.raises(ValueError) as e:
            build_model('yolov3_aleatoric', 64, 96, T=1, engine_options={'tta': bad})
        assert field in str(e.value)
    m = build_model('bayesian_yolov3_aleatoric', 64, 96, T=2, engine_options={'tta': {'flip': False, 'sizes': [[96, 128]]}})[1]
    geom = m.tta.geometry()
    assert [(g[0], g[1]) for g in geom] == [(2, 3), (4, 6), (8, 12), (3, 4), (6, 8), (12, 16)]
    for (_, _, own), (_, _, other) in zip(geom[:3], geom[3:]):           # priors * (full / size): the same box in pixels of the larger frame
        for (ph, pw), (qh, qw) in zip(own, other):
            assert qh == ph * (64 / 96.0) and qw == pw * (96 / 128.0)
    for kw, field in ((dict(t_shard=(0, 1)), 't_shard'), (dict(mask_bits=object()), 'mask_bits'), (dict(want_nms=False), 'want_nms')):
        with pytest.raises(ValueError) as e:
            m.run(None, **kw)
        assert field in str(e.value)
    m.engine.close()


def test_evaluate_config_keys():
    """tta / tta_compare of evaluate.py: absent keys stay absent, tta_compare is one comparison per run, bad settings name the field."""
    import evaluate
    from lib_yolo import yolov3
    base = {'full_img_size': [64, 96, 3], 'cls_cnt': 2, 'batch_size': 2, 'crop': False, 'priors': yolov3.ECP_9_PRIORS, 'T': 4,
            'implicit_background_class': True, 'weights': 'synthetic', 'data': {'file_pattern': 'x-*'}, 'out_path': 'x'}
    c = evaluate.check_config(base, 'aleatoric')
    assert 'tta' not in c and 'tta_compare' not in c and 'tta' not in c.get('engine_options', {})
    c = evaluate.check_config(dict(base, tta={'flip': True, 'sizes': [[96, 128]]}), 'aleatoric')
    assert c['engine_options']['tta'] == {'flip': True, 'sizes': [[96, 128]]} and c['tta_compare'] is False
    c = evaluate.check_config(dict(base, tta_compare=True), 'aleatoric')
    assert c['tta'] is True and 'tta' not in c.get('engine_options', {})
    for extra in (dict(box_vote=True, box_vote_compare=True), dict(soft_nms_compare=True)):
        with pytest.raises(ValueError) as e:
            evaluate.check_config(dict(base, tta_compare=True, **extra), 'aleatoric')
        assert 'tta_compare together with' in str(e.value) and 'one comparison per run' in str(e.value)
        with pytest.raises(ValueError):
            evaluate.check_config(dict(base, tta=True, **extra), 'aleatoric')
    with pytest.raises(ValueError) as e:
        evaluate.check_config(dict(base, tta=True, t_ladder=[1, 2]), 'bayesian')
    assert 't_ladder together with tta' in str(e.value)
    with pytest.raises(ValueError) as e:
        evaluate.check_config(dict(base, tta={'sizes': [[96, 100]]}), 'aleatoric')
    assert 'sizes[0]' in str(e.value)
    with pytest.raises(ValueError):
        evaluate.check_config(dict(base, tta_compare='yes'), 'aleatoric')


# ---- the C-ABI: struct and refusals (nothing is launched) -------------------------------------------------------------------------------
def test_support_cfg_struct_matches_the_header():
    from byolo import _lib
    text = open(os.path.join(REPO, 'include', 'byolo.h')).read()
    body = re.search(r'typedef struct byolo_tta_support_cfg \{(.*?)\} byolo_tta_support_cfg;', text, flags=re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    names = []
    for decl in body.split(';'):
        if decl.strip():
            ty, rest = decl.strip().split(None, 1)
            names += [(n.strip().split('[')[0], ty) for n in rest.split(',')]
    assert names == [('struct_bytes', 'int32_t'), ('n_views', 'int32_t'), ('iou_min', 'float'), ('min_score', 'float'), ('view_off', 'int32_t')]
    assert [n for n, _ in _lib.TtaSupportCfg._fields_] == [n for n, _ in names]
    assert int(re.search(r'#define BYOLO_TTA_MAX_VIEWS (\d+)', text).group(1)) == _lib.TTA_MAX_VIEWS == 8
    assert ctypes.sizeof(_lib.TtaSupportCfg) == 16 + 4 * 9


def _err():
    from byolo import _lib
    return _lib.lib.byolo_last_error(None).decode()


def test_merge_and_view_refuse_bad_arguments():
    from byolo import _lib
    lib = _lib.lib
    buf = np.zeros(4096, F32)
    p, q = ctypes.c_void_p(buf.ctypes.data), ctypes.c_void_p(buf.ctypes.data + 8192)
    merge = lambda src, B, Nv, D, kind, lc, flip, g, dst, Nu, off: lib.byolo_tta_merge(src, B, Nv, D, kind, lc, flip, g, dst, Nu, off, None)
    for args, field in (((p, 1, 4, 5, 0, -1, 0, 0, q, 8, 0), 'D 5'), ((p, 1, 4, 14, 1, 12, 0, 0, q, 8, 0), 'D 14'), ((p, 1, 4, 150, 2, 148, 0, 0, q, 8, 0), 'D 150'),
                        ((p, 1, 4, 16, 1, 13, 0, 0, q, 8, 0), 'layer_col'), ((p, 1, 4, 7, 0, 5, 0, 0, q, 8, 0), 'layer_col'),
                        ((p, 1, 4, 16, 1, 14, 0, 0, q, 8, 5), 'row_off'), ((p, 1, 4, 16, 1, 14, 0, 0, q, 3, 0), 'row_off'),
                        ((p, 1, 4, 16, 1, 14, 2, 0, q, 8, 0), 'flip'), ((p, 1, 4, 16, 1, 14, 0, 2, q, 8, 0), 'size_idx'), ((p, 1, 4, 16, 3, 14, 0, 0, q, 8, 0), 'kind'),
                        ((None, 1, 4, 16, 1, 14, 0, 0, q, 8, 0), 'd_rows is NULL'), ((p, 1, 4, 16, 1, 14, 0, 0, None, 8, 0), 'd_union is NULL'),
                        ((ctypes.c_void_p(buf.ctypes.data + 2), 1, 4, 16, 1, 14, 0, 0, q, 8, 0), 'd_rows must be 4-byte aligned'),
                        ((p, 1, 4, 16, 1, 14, 0, 0, ctypes.c_void_p(buf.ctypes.data + 8193), 8, 0), 'd_union must be 4-byte aligned'),
                        ((p, 1, 4, 16, 1, 14, 0, 0, ctypes.c_void_p(buf.ctypes.data + 64), 8, 0), 'overlaps')):
        assert merge(*args) == _lib.ERR_ARG and field in _err(), (args[1:8], _err())
    assert merge(None, 0, 4, 16, 1, 14, 0, 0, None, 8, 0) == 0 and merge(None, 1, 0, 16, 1, 14, 0, 0, None, 8, 0) == 0      # no-ops
    view = lambda src, B, sh, sw, flip, oh, ow, dst: lib.byolo_tta_view_f32(src, B, sh, sw, flip, oh, ow, dst, None)
    for args, field in (((None, 1, 4, 4, 0, 4, 4, q), 'NULL'), ((p, 1, 0, 4, 0, 4, 4, q), 'sizes'), ((p, 1, 4, 4, 3, 4, 4, q), 'flip'),
                        ((p, 1, 4, 4, 0, 4, 4, ctypes.c_void_p(buf.ctypes.data + 16)), 'overlaps')):
        assert view(*args) == _lib.ERR_ARG and field in _err(), _err()
    assert view(None, 0, 4, 4, 0, 4, 4, None) == 0


def test_support_refuses_a_bad_cfg():
    from byolo import _lib
    from conftest import build_model
    lib = _lib.lib
    m = build_model('yolov3_aleatoric', 64, 96, T=1, cls_cnt=3)[1]
    buf = np.zeros(65536, F32)
    p = lambda k: ctypes.c_void_p(buf.ctypes.data + 4096 * k)

    def call(cfg, Nu=16, D=17, ws_bytes=None, mode=2):
        need = lib.byolo_tta_support_workspace_bytes(2, Nu)
        return lib.byolo_tta_support(m.engine._h, p(0), 2, Nu, D, 9, 11, mode, ctypes.byref(cfg), p(1), p(2), 4, p(3), p(4), p(5), p(6), p(7),
                                     need if ws_bytes is None else ws_bytes, None)

    def cfg(**kw):
        c = _lib.TtaSupportCfg(struct_bytes=ctypes.sizeof(_lib.TtaSupportCfg), n_views=2, iou_min=0.5, min_score=0.001)
        c.view_off[1], c.view_off[2] = 8, 16
        for k, v in kw.items():
            if k == 'off':
                for i, o in enumerate(v):
                    c.view_off[i] = o
            else:
                setattr(c, k, v)
        return c
    err = lambda: lib.byolo_last_error(m.engine._h).decode()
    for c, field in ((cfg(struct_bytes=48), 'struct_bytes'), (cfg(n_views=0), 'n_views'), (cfg(n_views=9), 'n_views'), (cfg(off=[0, 9, 8]), 'view_off[2]'),
                     (cfg(off=[0, 8, 17]), 'view_off[2]'), (cfg(off=[1, 8, 16]), 'view_off[0]'), (cfg(iou_min=float('nan')), 'iou_min'),
                     (cfg(iou_min=-1.0), 'iou_min'), (cfg(min_score=float('nan')), 'min_score')):
        assert call(c) == _lib.ERR_ARG and field in err(), err()
    assert call(cfg(), mode=3) == _lib.ERR_ARG and 'nms_mode' in err()
    assert call(cfg(), D=12) == _lib.ERR_ARG and 'cls_start_idx' in err()
    assert call(cfg(), ws_bytes=16) == _lib.ERR_NOMEM and 'workspace' in err()
    assert lib.byolo_tta_support_workspace_bytes(0, 16) == 0 and lib.byolo_tta_support_workspace_bytes(2, 0) == 0
    m.engine.close()
