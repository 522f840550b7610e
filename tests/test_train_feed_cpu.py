"""The training feed without a GPU: the restatement of csrc/augment.hip (tests/_augment_ref.py) against hand-worked values, the
host-side box arithmetic and plan draws of byolo/augment.py, the record stream of lib_yolo.dataset_utils, the checkpoint names
of lib_yolo.train, the scripts' config keys, and the settings that are refused."""
import ast
import ctypes
import os
import re

import numpy as np
import pytest

import _augment_ref as ar
from conftest import REPO, PKG, golden

f32 = np.float32


# ---- restatement self-checks ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rgb", [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (0, 1, 1), (1, 0, 1)])
def test_saturation_of_pure_colours(rgb):
    x = np.array([rgb], f32)
    assert np.array_equal(ar.adjust_saturation(x, 1.0), x)                   # factor 1: unchanged
    assert np.array_equal(ar.adjust_saturation(x, 0.0), np.ones_like(x))      # saturation 0: grey at v = 1
    assert np.array_equal(ar.adjust_saturation(x, 1.5), x)                    # s clamps at 1


def test_saturation_grey_black_and_half():
    grey = np.array([[0.5, 0.5, 0.5]], f32)
    assert np.array_equal(ar.adjust_saturation(grey, 1.4), grey)              # range 0: h = 0, s = 0
    black = np.zeros((1, 3), f32)
    assert np.array_equal(ar.adjust_saturation(black, 1.4), black)            # v = 0: s = 0
    # (1, .5, .5): h = 0, s = .5, v = 1; factor .5 -> s = .25: (1, .75, .75)
    assert np.array_equal(ar.adjust_saturation(np.array([[1, .5, .5]], f32), 0.5), np.array([[1, .75, .75]], f32))


def test_hue_primaries_and_wrapping():
    red = np.array([[1, 0, 0]], f32)
    assert np.array_equal(ar.adjust_hue(red, 0.0), red)
    # + 1/6 of the circle: red -> yellow (h 0 -> 1); - 1/6: red -> magenta (h 0 -> -1 -> 5)
    third = f32(1.0) / f32(6.0)
    assert np.allclose(ar.adjust_hue(red, third), [[1, 1, 0]], atol=1e-6)
    assert np.allclose(ar.adjust_hue(red, -third), [[1, 0, 1]], atol=1e-6)
    blue = np.array([[0, 0, 1]], f32)                                         # h = 4 -> + 2 wraps at 6 to 0: red
    assert np.allclose(ar.adjust_hue(blue, 2 * third), [[1, 0, 0]], atol=1e-6)
    grey = np.array([[0.3, 0.3, 0.3]], f32)                                   # v_max == v_min: kept
    assert np.array_equal(ar.adjust_hue(grey, 0.17), grey)
    # the pixel's min and max are kept
    x = np.random.default_rng(0).random((50, 3)).astype(f32)
    y = ar.adjust_hue(x, 0.13)
    assert np.array_equal(np.sort(x, 1)[:, [0, 2]], np.sort(y, 1)[:, [0, 2]])


def test_bilinear_2x2_to_3x3_and_3x3_to_2x2():
    a = np.array([[0, 1], [2, 3]], f32)[..., None].repeat(3, -1)
    up = ar.resize_bilinear(a, 3, 3)[..., 0]
    # src = dst * 2/3: 0, .6667, 1.3333 -> lo 0, 0, 1 (hi clamped to 1); lerp 0, 2/3, 1/3 (the last row / column clamp)
    s = f32(2) / f32(3)
    l1 = f32(1) * s
    l2 = f32(2) * s - f32(1)
    row0 = [f32(0), f32(0) + (f32(1) - f32(0)) * l1, f32(1) + (f32(1) - f32(1)) * l2]
    assert np.array_equal(up[0], np.array(row0, f32))
    assert up[2, 2] == f32(3) and up[1, 0] == f32(0) + (f32(2) - f32(0)) * l1
    b = np.arange(9, dtype=f32).reshape(3, 3)[..., None].repeat(3, -1)
    down = ar.resize_bilinear(b, 2, 2)[..., 0]
    # src = dst * 1.5: 0, 1.5 -> rows 0 and (3 + 6) / 2, columns 0 and (x + x+1) / 2
    assert np.array_equal(down, np.array([[0, 1.5], [4.5, 6]], f32))


def test_blur_k2_bottom_right_border():
    x = np.ones((3, 4, 3), f32)
    y = ar.blur(x, 2)
    q = f32(0.25)
    assert y[0, 0, 0] == f32(1)
    assert y[2, 3, 0] == q                                                    # three zeros padded after: one of four
    assert y[2, 0, 0] == f32(0) + q + q + f32(0) * q + f32(0) * q                 # last row: two of four
    assert y[0, 3, 0] == f32(0.5)
    z = ar.blur(x, 3)
    assert z[0, 0, 0] == f32(4) * (f32(1) / f32(9)) or np.isclose(z[0, 0, 0], 4 / 9)
    assert z[1, 1, 0] == ar.blur(np.ones((3, 3, 3), f32), 3)[1, 1, 0]


def test_hash_stream_rates():
    u = ar.uniform(0xDEADBEEF12345678, np.arange(200000, dtype=np.uint32), ar.P_SALT)
    assert u.min() >= 0 and u.max() < 1 and abs(u.mean() - 0.5) < 0.005
    v = ar.uniform(0xDEADBEEF12345678, np.arange(200000, dtype=np.uint32), ar.P_PEPPER)
    assert abs(np.corrcoef(u, v)[0, 1]) < 0.01
    z = ar.gaussian(7, np.arange(200000, dtype=np.uint32))
    assert abs(z.mean()) < 0.01 and abs(z.std() - 1) < 0.01


# ---- boxes ------------------------------------------------------------------------------------------------------------------
def test_crop_boxes_hand_cases():
    from byolo import augment
    win = (f32(0.25), f32(0.25), f32(0.75), f32(0.75))
    boxes = np.array([[0.3, 0.3, 0.5, 0.6],          # inside
                      [0.0, 0.0, 0.1, 0.1],          # fully outside
                      [0.4, 0.4, 0.4, 0.6],          # zero area: NaN ratio, dropped
                      [0.25, 0.0, 0.75, 0.5],        # exactly half inside: kept
                      [0.25, 0.125, 0.75, 0.375],    # exactly half inside
                      [0.25, 0.0, 0.75, 0.3125]], f32)   # 0.0625 / 0.3125 = 20 %: dropped
    labels = np.arange(6, dtype=np.int32)
    out, lab = augment.crop_boxes(boxes, labels, *win)
    assert list(lab) == [0, 3, 4]
    assert np.array_equal(out[0], np.array([(f32(.3) - f32(.25)) / f32(.5), (f32(.3) - f32(.25)) / f32(.5),
                                            (f32(.5) - f32(.25)) / f32(.5), (f32(.6) - f32(.25)) / f32(.5)], f32))
    # exactly 25 % of the area inside is NOT kept (strictly greater)
    quarter = np.array([[0.0, 0.0, 0.5, 0.5]], f32)
    _, lab = augment.crop_boxes(quarter, np.array([9]), f32(0.25), f32(0.25), f32(0.75), f32(0.75))
    assert len(lab) == 0
    _, lab = augment.crop_boxes(quarter, np.array([9]), f32(0.25), f32(0.0), f32(0.75), f32(0.75))
    assert list(lab) == [9]                                                   # 50 %


def test_flip_boxes():
    from byolo import augment
    b = np.array([[0.1, 0.2, 0.3, 0.5]], f32)
    assert np.array_equal(augment.flip_boxes(b), np.array([[0.1, f32(1) - f32(0.5), 0.3, f32(1) - f32(0.2)]], f32))


# ---- plan statistics --------------------------------------------------------------------------------------------------------
def test_plan_statistics_over_20000_draws():
    from byolo import augment
    cfg = {'crop': True, 'crop_img_size': [96, 160, 3], 'full_img_size': [192, 320, 3], 'seed': 5}
    N = 20000
    p = augment.empty_plans(N)
    scales = []
    for i in range(N):
        augment.draw(cfg, 'train', 0, i, p[i])
        if p[i]['rescale']:
            scales.append(p[i]['ch'] / 96.0 - 1)
    assert abs(p['flip'].mean() - 0.5) < 0.01
    for f in ('blur_k', 'color_op', 'noise_op'):
        assert abs((p[f] > 0).mean() - 0.05) < 0.005, f
    assert abs(p['rescale'].mean() - 0.33) < 0.01
    for f, vals in (('blur_k', (2, 3)), ('color_op', (1, 2, 3)), ('noise_op', (1, 2, 3))):
        sel = p[f][p[f] > 0]
        for v in vals:
            assert abs((sel == v).mean() - 1.0 / len(vals)) < 0.07, (f, v)
    scales = np.array(scales)
    # N(0, 0.5) clipped at +-0.7: P(|z| > 1.4) = 0.1615; ch truncates, so the top end shows as ch = int(1.7 * 96) = 163
    clip_mass = np.mean((p['ch'][p['rescale'] == 1] == int(f32(1.7) * f32(96))) | (p['ch'][p['rescale'] == 1] == int(f32(0.3) * f32(96))))
    assert abs(clip_mass - 0.16) < 0.02
    assert (p['y0'] >= 0).all() and (p['x0'] >= 0).all()
    assert (p['y0'] + p['ch'] <= 192).all() and (p['x0'] + p['cw'] <= 320).all()
    plain = p[p['rescale'] == 0]
    assert plain['x0'].min() == 0 and plain['x0'].max() == 320 - 160                       # both ends of x reached
    assert (plain['ch'] == 96).all() and (plain['cw'] == 160).all()
    # the draws are a pure function of (seed, split, epoch, position)
    q = augment.empty_plans(1)
    augment.draw(cfg, 'train', 0, 1234, q[0])
    assert q[0].tobytes() == p[1234].tobytes()
    augment.draw(cfg, 'val', 0, 1234, q[0])
    assert q[0]['flip'] == 0 and q[0]['blur_k'] == 0 and q[0]['color_op'] == 0 and q[0]['noise_op'] == 0


# ---- record stream ----------------------------------------------------------------------------------------------------------
def _synthetic_set(tmp_path, files=3, records=7):
    from lib_yolo import dataset_utils as du
    for f in range(files):
        du.write_tfrecords(str(tmp_path / ('set-%d-of-%d' % (f, files))),
                           [du.make_example({'image/filename': 'f%d_r%d' % (f, r)}) for r in range(records)])
    return {'seed': 3, 'train': {'file_pattern': str(tmp_path / 'set-*'), 'num_shards': 3, 'shuffle_buffer_size': 5, 'cache': True}}


def test_record_stream_epochs(tmp_path):
    from lib_yolo import dataset_utils as du
    cfg = _synthetic_set(tmp_path)
    s = du.create_dataset(cfg, 'train')
    orders = [list(s.epoch(e)) for e in range(3)]
    for o in orders:
        assert len(o) == 21 and len(set(o)) == 21                              # every record once per epoch
    assert orders[0] != orders[1] and orders[1] != orders[2]                  # reshuffled each epoch
    again = du.create_dataset(cfg, 'train')
    assert [list(again.epoch(e)) for e in range(3)] == orders                 # same seed, same order
    other = du.create_dataset(dict(cfg, seed=4), 'train')
    assert list(other.epoch(0)) != orders[0]
    it = iter(s)
    head = [next(it) for _ in range(23)]
    assert [h[:2] for h in head[:2]] == [(0, 0), (0, 1)] and head[21][:2] == (1, 0)     # repeat: epoch 1 follows
    names = {du.parse_example(s.payload(r))['image/filename'][0] for r in orders[0]}
    assert len(names) == 21


def test_parse_fn_boxes_and_label_shift():
    from lib_yolo import dataset_utils as du
    import struct

    def floats(name, vals):
        return name, vals
    # a tf.train.Example with float and int64 lists, written by hand
    def pb(num, payload):
        def vi(x):
            o = b''
            while True:
                b = x & 0x7F
                x >>= 7
                o += bytes([b | (0x80 if x else 0)])
                if not x:
                    return o
        return vi((num << 3) | 2) + vi(len(payload)) + payload
    feats = b''
    for name, vals in (('image/object/bbox/ymin', [0.1, 0.2]), ('image/object/bbox/xmin', [0.3, 0.4]),
                       ('image/object/bbox/ymax', [0.5, 0.6]), ('image/object/bbox/xmax', [0.7, 0.8])):
        feats += pb(1, pb(1, name.encode()) + pb(2, pb(2, pb(1, struct.pack('<2f', *vals)))))
    feats += pb(1, pb(1, b'image/object/class/label') + pb(2, pb(3, pb(1, bytes([1, 2])))))
    feats += pb(1, pb(1, b'image/encoded') + pb(2, pb(1, pb(1, b'PNGDATA'))))
    ex = pb(1, feats)
    enc, boxes, labels = du.make_parse_fn({'implicit_background_class': True})(ex)
    assert enc == b'PNGDATA'
    assert np.array_equal(boxes, np.array([[0.1, 0.3, 0.5, 0.7], [0.2, 0.4, 0.6, 0.8]], f32))
    assert list(labels) == [0, 1]
    _, _, labels = du.make_parse_fn({'implicit_background_class': False})(ex)
    assert list(labels) == [1, 2]


# ---- structs, checkpoints, scripts ------------------------------------------------------------------------------------------
def test_aug_plan_struct_matches_the_header():
    from byolo import _lib, augment
    text = open(os.path.join(REPO, "include", "byolo.h")).read()
    body = re.search(r"typedef struct byolo_aug_plan \{(.*?)\} byolo_aug_plan;", text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    types = {"int32_t": ctypes.c_int32, "float": ctypes.c_float, "uint64_t": ctypes.c_uint64}
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ty, names = decl.split(None, 1)
            fields += [(n.strip(), types[ty]) for n in names.split(",")]
    assert fields == list(_lib.AugPlan._fields_)
    assert ctypes.sizeof(_lib.AugPlan) == 56 == augment.PLAN_DTYPE.itemsize
    for n, _ in fields:
        assert augment.PLAN_DTYPE.fields[n][1] == getattr(_lib.AugPlan, n).offset


def test_checkpoint_names_round_trip(tmp_path):
    from byolo import tf_checkpoint
    from lib_yolo import train

    class FakeEngine:
        def get_params(self):
            return {'darknet/conv_0/conv2d/kernel': np.ones((3, 3, 3, 32), f32), 'det_net_1/conv_1/conv2d/kernel': np.zeros((1, 1, 2, 2), f32),
                    'det_net_1/conv_1/batch_normalization/moving_mean': np.zeros(2, f32)}

    class FakeTrainer:
        engine = FakeEngine()

        def variables(self):
            return {'det_net_1/conv_1/conv2d/kernel': (1, 1, 2, 2)}

        def moving_statistics(self):
            return {'det_net_1/conv_1/batch_normalization/moving_mean': (2,)}

        def state_dict(self):
            k = 'det_net_1/conv_1/conv2d/kernel'
            return {k: np.full((1, 1, 2, 2), 2, f32), k + '/Adam': np.full((1, 1, 2, 2), 3, f32),
                    k + '/Adam_1': np.full((1, 1, 2, 2), 4, f32),
                    'det_net_1/conv_1/batch_normalization/moving_mean': np.full(2, 5, f32), 'global_step': np.int64(7)}

    s = train.Saver(FakeTrainer(), str(tmp_path), 'run', 2)
    for step in (5, 6, 7):
        s.save(step)
    assert sorted(os.path.basename(p) for p in tmp_path.glob('*.index')) == ['run-6.index', 'run-7.index']
    state = open(tmp_path / 'checkpoint').read()
    assert 'model_checkpoint_path: "run-7"' in state and state.count('all_model_checkpoint_paths') == 2
    assert train.latest_checkpoint(str(tmp_path)) == str(tmp_path / 'run-7')
    got = tf_checkpoint.read(str(tmp_path / 'run-7'))
    assert sorted(got) == sorted(['darknet/conv_0/conv2d/kernel', 'det_net_1/conv_1/conv2d/kernel',
                                  'det_net_1/conv_1/batch_normalization/moving_mean', 'optimizer/det_net_1/conv_1/conv2d/kernel/Adam',
                                  'optimizer/det_net_1/conv_1/conv2d/kernel/Adam_1', 'optimizer/beta1_power', 'optimizer/beta2_power'])
    assert (got['optimizer/det_net_1/conv_1/conv2d/kernel/Adam_1'] == 4).all()
    b1, b2 = f32(0.9), f32(0.999)                                   # TF1 Adam: float32 running products, one factor per update
    for _ in range(7):
        b1, b2 = f32(b1 * f32(0.9)), f32(b2 * f32(0.999))
    assert got['optimizer/beta1_power'] == b1 and got['optimizer/beta2_power'] == b2
    assert got['det_net_1/conv_1/conv2d/kernel'][0, 0, 0, 0] == 2


def _script_config(path):
    tree = ast.parse(open(path).read())
    for node in ast.walk(tree):
        if isinstance(node, ast.Assign) and getattr(node.targets[0], 'id', None) == 'config' and isinstance(node.value, ast.Dict):
            out = {}
            for k, v in zip(node.value.keys, node.value.values):
                if isinstance(v, ast.Dict):
                    out.update({'%s.%s' % (k.value, k2.value): ast.unparse(v2) for k2, v2 in zip(v.keys, v.values)})
                else:
                    out[k.value] = ast.unparse(v)
            return out


def test_scripts_config_keys_match_the_fixture():
    fx = golden('training_configs.json')
    assert sorted(fx) == ['pretraining.py', 'uncertainty_training.py', 'yolov3_training.py']
    for name, ref in fx.items():
        assert _script_config(os.path.join(PKG, name)) == ref, name


def test_refused_settings():
    from lib_yolo import train, utils, yolov3
    with pytest.raises(NotImplementedError, match='freeze_darknet53'):
        train.build(yolov3.yolov3, {'freeze_darknet53': False})
    with pytest.raises(NotImplementedError, match='qualitative_eval'):
        utils.qualitative_eval(yolov3.yolov3, {'training': False})


def test_add_file_logging(tmp_path):
    import logging
    from lib_yolo import utils
    cfg = {'log_path': str(tmp_path / 'log'), 'run_id': 'r'}
    h = utils.add_file_logging(cfg)
    try:
        logging.getLogger('').warning('hello %d', 1)
        h.flush()
        assert 'hello 1' in open(tmp_path / 'log' / 'r.log').read()
        with pytest.raises(RuntimeError):
            utils.add_file_logging(cfg)
    finally:
        logging.getLogger('').removeHandler(h)
        h.close()
