"""The training feed on the device: csrc/augment.hip against the float32 restatement of tests/_augment_ref.py (bit-identical
except the Gaussian term), the TFRecord feed of lib_yolo.dataset_utils.TrainValDataset, and lib_yolo.train.start end to end
(logging, validation, checkpoints the inference side loads, resume)."""
import glob
import io
import json
import logging
import os
import re

import numpy as np
import pytest
import torch

import _augment_ref as ar

pytestmark = pytest.mark.gpu

FH, FW, OH, OW = 37, 53, 29, 41


def _plans(rows):
    from byolo import augment
    p = augment.empty_plans(len(rows))
    for k, r in enumerate(rows):
        base = dict(y0=3, x0=5, ch=OH, cw=OW, noise_key=0x123456789ABCDEF0 + k)
        base.update(r)
        for f, v in base.items():
            p[k][f] = v
    return p


def _frames(n, seed=0, h=FH, w=FW):
    return np.random.default_rng(seed).integers(0, 256, (n, h, w, 3), dtype=np.uint8)


def _run(frames, plans, oh=OH, ow=OW):
    from byolo import augment
    out = augment.augment_batch(torch.from_numpy(frames).cuda(), plans, (oh, ow))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _check(got, frames, plans, oh=OH, ow=OW):
    for b in range(len(plans)):
        ref = ar.augment_one(frames[b], plans[b], oh, ow)
        if int(plans[b]['noise_op']) == 3:
            assert np.abs(got[b].astype(np.float64) - ref).max() <= 1e-6, b
        else:
            assert np.array_equal(got[b].view(np.uint32), ref.view(np.uint32)), \
                (b, plans[b], np.argwhere(got[b] != ref)[:5], np.abs(got[b] - ref).max())


SINGLE = [
    {}, {"flip": 1}, {"blur_k": 2}, {"blur_k": 3}, {"color_op": 1, "color_param": 1.37}, {"color_op": 1, "color_param": 0.55},
    {"color_op": 2, "color_param": -0.17}, {"color_op": 3, "color_param": 0.19}, {"color_op": 3, "color_param": -0.2},
    {"noise_op": 1, "noise_param": 0.03}, {"noise_op": 2, "noise_param": 0.03}, {"noise_op": 3, "noise_param": 0.04},
    {"rescale": 1, "y0": 0, "x0": 0, "ch": FH, "cw": FW},             # down
    {"rescale": 1, "y0": 7, "x0": 11, "ch": 13, "cw": 22},             # up
    {"rescale": 1, "y0": 2, "x0": 1, "ch": 29, "cw": 50},              # up in y, down in x
]
COMBOS = [
    {"flip": 1, "blur_k": 2}, {"flip": 1, "blur_k": 3, "color_op": 3, "color_param": 0.11, "noise_op": 3, "noise_param": 0.05},
    {"rescale": 1, "y0": 4, "x0": 9, "ch": 17, "cw": 31, "flip": 1, "blur_k": 2, "color_op": 1, "color_param": 1.49,
     "noise_op": 2, "noise_param": 0.008},
    {"rescale": 1, "y0": 0, "x0": 2, "ch": 36, "cw": 50, "blur_k": 3, "color_op": 2, "color_param": 0.2, "noise_op": 1,
     "noise_param": 0.0051},
]


@pytest.mark.parametrize("row", SINGLE + COMBOS)
def test_kernel_matches_the_restatement(row):
    plans = _plans([row])
    frames = _frames(1, seed=len(str(row)))
    _check(_run(frames, plans), frames, plans)


def test_one_launch_with_a_plan_per_image_and_position_independence():
    rows = SINGLE + COMBOS
    plans = _plans(rows)
    frames = _frames(len(rows), seed=3)
    got = _run(frames, plans)
    _check(got, frames, plans)
    again = _run(frames, plans)
    assert np.array_equal(got.view(np.uint32), again.view(np.uint32))               # deterministic
    for b in (0, 5, len(rows) - 1):
        alone = _run(frames[b:b + 1], plans[b:b + 1])
        assert np.array_equal(alone[0].view(np.uint32), got[b].view(np.uint32))


def test_large_batch_and_shipped_row_band():
    """More than 32 images (several launches), and frames shipped as the row band their crop reads (row0)."""
    rows = [dict(r) for r in (SINGLE + COMBOS) * 2][:34]
    plans = _plans(rows)
    frames = _frames(len(rows), seed=9)
    full = _run(frames, plans)
    lo = int(min(plans['y0']))
    hi = int(max(plans['y0'] + plans['ch']))
    band = np.ascontiguousarray(frames[:, lo:hi])
    plans_b = plans.copy()
    plans_b['row0'] = lo
    got = _run(band, plans_b)
    assert np.array_equal(full.view(np.uint32), got.view(np.uint32))
    _check(full, frames, plans)


def test_out_of_range_plans_are_refused():
    from byolo import _lib
    frames = torch.from_numpy(_frames(1)).cuda()
    from byolo import augment
    for bad in ({"y0": FH - OH + 1}, {"x0": -1}, {"blur_k": 1}, {"color_op": 4}, {"noise_op": 7}, {"flip": 2},
                {"ch": OH - 1}, {"rescale": 1, "ch": FH, "cw": FW + 1}, {"row0": 4},
                # parameters the hue op's wrap loops could not finish with, and non-finite ones
                {"color_op": 3, "color_param": 1.5}, {"color_op": 3, "color_param": -3e7}, {"color_op": 3, "color_param": float("inf")},
                {"color_op": 1, "color_param": float("nan")}, {"color_op": 2, "color_param": float("-inf")},
                {"noise_op": 3, "noise_param": float("inf")}, {"noise_op": 1, "noise_param": float("nan")}):
        with pytest.raises(_lib.ByoloError) as e:
            augment.augment_batch(frames, _plans([bad]), (OH, OW))
        assert e.value.code == _lib.ERR_ARG, bad


WIDE = [  # 37 x 141 output: three tile rows and three tile columns, rows of 423 floats (not a multiple of 4)
    {"blur_k": 2, "flip": 1}, {"blur_k": 3, "flip": 1}, {"blur_k": 3}, {"blur_k": 2},
    {"blur_k": 3, "flip": 1, "rescale": 1, "y0": 2, "x0": 7, "ch": 41, "cw": 120, "color_op": 3, "color_param": -0.13},
    {"blur_k": 2, "rescale": 1, "y0": 0, "x0": 0, "ch": 45, "cw": 150, "noise_op": 2, "noise_param": 0.02}, {"flip": 1},
]


def test_wide_rows_tile_halos_and_unaligned_row_starts():
    """Blur halos across tile borders (columns and rows) and rows that start inside a 16-byte slot (j0 > 0, lead != 0)."""
    plans = _plans([dict(r, y0=r.get("y0", 4), x0=r.get("x0", 5), ch=r.get("ch", 37), cw=r.get("cw", 141)) for r in WIDE])
    frames = _frames(len(WIDE), seed=21, h=45, w=150)
    got = _run(frames, plans, 37, 141)
    _check(got, frames, plans, 37, 141)
    one = _run(frames[1:2], plans[1:2], 37, 141)                     # an odd image offset in the batch moves every row's lead
    assert np.array_equal(one[0].view(np.uint32), got[1].view(np.uint32))


def test_data_augmentation_methods_against_the_restatement():
    from byolo import augment
    from lib_yolo import data_augmentation as da
    fr = _frames(1, seed=31, h=64, w=96)[0]
    img = torch.from_numpy(fr).cuda()
    f32img = torch.from_numpy(fr.astype(np.float32) * ar.K255).cuda()        # decode_img's float32 frame is accepted as well
    boxes = np.array([[0.1, 0.2, 0.5, 0.4], [0.6, 0.0, 0.9, 0.3]], np.float32)
    labels = np.array([0, 1], np.int32)
    aug = da.DataAugmenter((64, 96, 3), seed=5)

    def same(out, plan, oh=64, ow=96):
        torch.cuda.synchronize()
        ref = ar.augment_one(fr, plan, oh, ow)
        got = out.cpu().numpy()
        if int(plan['noise_op']) == 3:
            assert np.abs(got.astype(np.float64) - ref).max() <= 1e-6
        else:
            assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), plan

    for k in range(12):
        out, bx, lb = aug.augment(img if k % 2 else f32img, boxes, labels)
        same(out, aug.last_plan)
        exp_b, exp_l = augment.apply_to_boxes(aug.last_plan, None, boxes, labels)
        assert np.array_equal(bx, exp_b) and np.array_equal(lb, exp_l)
    out, bx = aug.flip_lr(img, boxes)
    same(out, aug.last_plan)
    assert aug.last_plan['flip'] == 1 and np.array_equal(bx, augment.flip_boxes(boxes))
    for name, field in (('blur', 'blur_k'), ('color_augmentations', 'color_op'), ('noise_augmentations', 'noise_op'),
                        ('colored_salt_n_pepper', 'noise_op'), ('salt_n_pepper', 'noise_op'), ('additive_gaussian_noise', 'noise_op')):
        out = getattr(aug, name)(img)
        assert int(aug.last_plan[field]) > 0, name
        same(out, aug.last_plan)
    with pytest.raises(ValueError):
        aug.blur(f32img + 0.001)                                               # not a decoded frame

    cropper = da.ImageCropper({'crop_img_size': [32, 48, 3], 'full_img_size': [64, 96, 3], 'seed': 3})
    for name in ('random_crop_and_sometimes_rescale', 'random_crop_with_rescale', 'random_crop', 'center_crop') * 2:
        out, bx, lb = getattr(cropper, name)(img, boxes, labels)
        p = cropper.last_plan
        assert out.shape == (32, 48, 3)
        same(out, p, 32, 48)
        if name == 'random_crop_with_rescale':
            assert p['rescale'] == 1
        if name in ('random_crop', 'center_crop'):
            assert p['rescale'] == 0
        y0, x0 = np.float32(p['y0']) / np.float32(64), np.float32(p['x0']) / np.float32(96)
        h = np.float32(p['ch']) / np.float32(64) if p['rescale'] else np.float32(32 / 64.0)
        w = np.float32(p['cw']) / np.float32(96) if p['rescale'] else np.float32(48 / 96.0)
        exp_b, exp_l = augment.crop_boxes(boxes, labels, y0, x0, y0 + h, x0 + w)
        assert np.array_equal(bx, exp_b) and np.array_equal(lb, exp_l)
    with pytest.raises(AssertionError):
        da.ImageCropper({'crop_img_size': [32, 32, 3], 'full_img_size': [64, 96, 3]})


# ---- the feed -------------------------------------------------------------------------------------------------------------
SH, SW, CH, CW, C = 192, 320, 96, 160, 2


@pytest.fixture(scope="module")
def shards(tmp_path_factory):
    from byolo import synth
    d = tmp_path_factory.mktemp("shards")
    train = synth.training_shards(str(d), 2, 6, SH, SW, seed=1)
    val = synth.training_shards(str(d), 1, 4, SH, SW, seed=2, prefix="val")
    return train, val, d


def _priors():
    # the ECP table at half size: cropping 192 x 320 frames to 96 x 160 doubles every prior, and the largest must stay below 1;
    # a table of its own per model, because building a cropped model rescales the table it is given in place (lib_yolo/model.py)
    from lib_yolo import data, yolov3
    return {s: [data.Prior(h=p.h * 0.5, w=p.w * 0.5) for p in prs] for s, prs in yolov3.ECP_9_PRIORS.items()}


def _config(shards, tmp, **kw):
    from lib_yolo import yolov3
    train, val, _ = shards
    cfg = {'training': True, 'resume_training': False, 'resume_checkpoint': 'last', 'priors': _priors(), 'run_id': 'run',
           'checkpoint_path': str(tmp / 'ckpt'), 'tensorboard_path': str(tmp / 'tb'), 'log_path': str(tmp / 'log'),
           'ckp_max_to_keep': 2, 'checkpoint_interval': 40, 'ign_thresh': 0.7, 'crop_img_size': [CH, CW, 3],
           'full_img_size': [SH, SW, 3], 'train_steps': 100, 'darknet53_weights': str(tmp / 'darknet53.weights'), 'batch_size': 2,
           'lr': 1e-4, 'cpu_thread_cnt': 1, 'crop': True, 'freeze_darknet53': True, 'aleatoric_loss': False, 'cls_cnt': C,
           'implicit_background_class': True, 'seed': 11,
           'train': {'file_pattern': train, 'num_shards': 2, 'shuffle_buffer_size': 5, 'cache': False},
           'val': {'file_pattern': val, 'num_shards': 1, 'shuffle_buffer_size': 3, 'cache': True}}
    cfg.update(kw)
    return cfg


def _decode(key, shape):
    from lib_yolo import dataset_utils as du
    s = du.RecordStream({'x': {'file_pattern': key[0]}}, 'x', 'train')
    enc, boxes, labels = du.make_parse_fn({'implicit_background_class': True})(s.payload((key[0], key[1])))
    return du.decode_png_u8(enc, shape), boxes, labels


def _batches(cfg, n_train, n_val):
    from lib_yolo import dataset_utils as du
    ds = du.TrainValDataset(None, cfg)
    try:
        tr = [next(ds.train) for _ in range(n_train)]
        va = [next(ds.val) for _ in range(n_val)]
        torch.cuda.synchronize()
        return [dict(b, img=b['img'].cpu().numpy()) for b in tr + va]
    finally:
        ds.close()


def test_feed_batches_equal_the_restatement(shards, tmp_path):
    from byolo import augment
    got = _batches(_config(shards, tmp_path), 7, 3)
    for b in got:
        frames, exp_boxes, exp_labels = [], [], []
        for k, key in enumerate(b['keys']):
            fr, bx, lb = _decode(key, (SH, SW, 3))
            frames.append(fr)
            p = b['plans'][k]
            win = (np.float32(p['y0']) / np.float32(SH), np.float32(p['x0']) / np.float32(SW))
            h = (np.float32(p['ch']) / np.float32(SH)) if p['rescale'] else np.float32(CH / float(SH))
            w = (np.float32(p['cw']) / np.float32(SW)) if p['rescale'] else np.float32(CW / float(SW))
            bx, lb = augment.apply_to_boxes(p, (win[0], win[1], win[0] + h, win[1] + w), bx, lb)
            exp_boxes.append(bx)
            exp_labels.append(lb)
        _check(b['img'], np.stack(frames), b['plans'], CH, CW)
        assert list(b['counts']) == [len(x) for x in exp_boxes]
        for k in range(len(frames)):
            n = int(b['counts'][k])
            assert np.array_equal(b['boxes'][k, :n], exp_boxes[k]) and np.array_equal(b['labels'][k, :n], exp_labels[k])
    # the same seed gives the same batches whatever the thread count
    again = _batches(_config(shards, tmp_path, cpu_thread_cnt=4), 7, 3)
    for a, b in zip(got, again):
        assert a['keys'] == b['keys'] and a['plans'].tobytes() == b['plans'].tobytes()
        assert np.array_equal(a['img'].view(np.uint32), b['img'].view(np.uint32))


def test_frame_of_the_wrong_size_names_the_record(shards, tmp_path):
    from lib_yolo import dataset_utils as du
    cfg = _config(shards, tmp_path, full_img_size=[SH, SW + 32, 3], crop_img_size=[CH, CW + 16, 3])
    ds = du.TrainValDataset(None, cfg)
    try:
        with pytest.raises(ValueError, match=r"record \d+: image shape"):
            next(ds.train)
    finally:
        ds.close()


# ---- train.start ------------------------------------------------------------------------------------------------------------
def _darknet(cfg, variant):
    from byolo import synth
    from lib_yolo import yolov3, darknet, model
    f = getattr(yolov3, variant)(dict(cfg, inference_mode=False, priors=_priors()))
    m = f.init_model(inputs=model.Placeholder((2, CH, CW, 3)), training=False).get_model()
    params = synth.base_params(m.engine.param_shapes(), variant, C, seed=7)
    stats = np.load(os.path.join(os.path.dirname(__file__), "golden", "bn_stats.npz"))
    params.update({k: stats[k].astype(np.float32) for k in stats.files if k in params})
    darknet.write_darknet_weights(m.layers[:f._darknet53_layer_cnt], cfg['darknet53_weights'], params)
    m.engine.close()


def _rows(model, img):
    out = model.run(img, seed=5)
    torch.cuda.synchronize()
    return out['boxes'].cpu().numpy()


def _log_lines(caplog):
    return [r.getMessage() for r in caplog.records]


def test_start_checkpoints_inference_and_resume(shards, tmp_path, caplog):
    from byolo import inference
    from conftest import build_model
    from lib_yolo import train, yolov3
    caplog.set_level(logging.INFO)
    cfg = _config(shards, tmp_path)
    _darknet(cfg, 'yolov3')
    tr = train.start(yolov3.yolov3, cfg)
    lines = _log_lines(caplog)
    for s in (25, 50, 75, 100):
        assert any(l.startswith('{:5d} train >>> total_loss:'.format(s)) for l in lines), s
    assert any(l.startswith('  100 val   >>> total_loss:') for l in lines)
    vals = [float(v) for l in lines if '>>>' in l for v in re.findall(r'[-\d.]+(?:e[-+]\d+)?(?=,|$)', l.split('>>>')[1])]
    assert vals and np.isfinite(vals).all()
    folder = tmp_path / 'ckpt' / 'run'
    assert sorted(p.name for p in folder.glob('*.index')) == ['run-100.index', 'run-80.index']      # ckp_max_to_keep = 2
    assert glob.glob(str(folder / 'config_*_run.json')) and json.load(open(glob.glob(str(folder / 'config_*_run.json'))[0]))['lr'] == 1e-4
    assert 'model_checkpoint_path: "run-100"' in open(folder / 'checkpoint').read()
    assert tr.step_count == 100

    # the last checkpoint in a fresh inference model = the trainer's variables handed over directly
    img = torch.from_numpy(np.random.default_rng(3).random((2, CH, CW, 3), dtype=np.float32)).cuda()
    _, a = build_model('yolov3', CH, CW, B=2)
    ck = inference.find_checkpoint({'checkpoint_path': str(tmp_path / 'ckpt'), 'run_id': 'run', 'step': 'last'})
    assert ck.endswith('run-100.index')
    inference.restore(a, ck)
    yb, b = build_model('yolov3', CH, CW, B=2)                         # backbone from the Darknet file, heads from the trainer
    yb.load_darknet53_weights(cfg['darknet53_weights'])
    tr.apply_to(b)
    assert np.array_equal(_rows(a, img).view(np.uint32), _rows(b, img).view(np.uint32))

    # resume from 'last': the same state, bit for bit; one more step on the same batch matches the uninterrupted trainer
    tr2 = train.start(yolov3.yolov3, _config(shards, tmp_path, resume_training=True, resume_checkpoint='last'))
    s1, s2 = tr.state_dict(), tr2.state_dict()
    assert sorted(s1) == sorted(s2)
    for k in s1:
        assert np.asarray(s1[k]).tobytes() == np.asarray(s2[k]).tobytes(), k
    boxes = np.array([[[0.2, 0.2, 0.5, 0.4]], [[0.1, 0.5, 0.3, 0.6]]], np.float32)
    labels = np.zeros((2, 1), np.int32)
    l1 = tr.step(img, boxes, labels, seed=111)
    l2 = tr2.step(img, boxes, labels, seed=111)
    assert l1 == l2
    s1, s2 = tr.state_dict(), tr2.state_dict()
    for k in s1:
        assert np.asarray(s1[k]).tobytes() == np.asarray(s2[k]).tobytes(), k
    for m in (a, b, tr.model, tr2.model):
        m.engine.close()


def test_bayesian_run_resumes_from_a_yolov3_aleatoric_checkpoint(shards, tmp_path, caplog):
    from lib_yolo import train, yolov3
    caplog.set_level(logging.INFO)
    cfg = _config(shards, tmp_path, run_id='pretraining', train_steps=25, checkpoint_interval=1000)
    _darknet(cfg, 'yolov3_aleatoric')
    pre = train.start(yolov3.yolov3_aleatoric, cfg)
    pre_state = pre.state_dict()
    ck = str(tmp_path / 'ckpt' / 'pretraining' / 'pretraining-25')
    assert os.path.exists(ck + '.index')
    bcfg = _config(shards, tmp_path, run_id='epi_ale', train_steps=125, checkpoint_interval=1000, inference_mode=False,
                   aleatoric_loss=True, resume_training=True, resume_checkpoint=ck, darknet53_weights=cfg['darknet53_weights'])
    tr = train.start(yolov3.bayesian_yolov3_aleatoric, bcfg)
    assert tr.step_count == 125
    lines = _log_lines(caplog)
    assert any(l.startswith('  125 train >>> ') for l in lines) and any(l.startswith('  100 val   >>> ') for l in lines)
    for l in lines:
        if '>>>' in l:
            assert 'nan' not in l and 'inf' not in l, l
    assert (tmp_path / 'ckpt' / 'epi_ale' / 'epi_ale-125.index').exists()
    shared = [k for k in tr.variables() if k in pre_state]
    assert shared
    for m in (pre.model, tr.model):
        m.engine.close()
