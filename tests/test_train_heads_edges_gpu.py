"""Head training on the device (byolo.train.HeadTrainer, csrc/train_heads.hip) against float64 on the hand-built graphs of
tests/_head_graphs.py, whose shapes land on the guards the real heads reach at no image size: ragged M in one tile and behind full
tiles, ragged wgrad slices, reduction lengths that end inside a BK step, Kc and N that are no multiples of 8, N across a column tile,
more than 256 channels, every kind of view, 1-wide and 1-pixel grids, the 32-bit padding of the dropout masks, the library's own
dropout stream.

The reference is tests/_heads_ref.py `grads` in float64 fed the DEVICE's taps; the bounds are those of tests/test_train_heads_gpu.py
(tests/_head_graphs.py `ratios`): raw outputs (and, in the dropout cases, every head activation) |dev - ref| <= 1e-4 * max(1, |ref|)
per element, the six losses within 1e-5 * |ref|, every gradient tensor max |dev - ref| <= max(1e-4 * max |ref|, 2 * d32) with d32
the same restatement run in float32; the update within 1e-6 * max(1, |ref|).  No exclusions; NaN / inf fail.
tests/test_train_heads_edges_cpu.py shows that each of ten one-line defects of the kernels lies at >= 4 x these bounds."""
import numpy as np
import pytest
import torch

from conftest import record_parity

import _head_graphs as G
import _heads_ref as hr
import _layer_ref as R

pytestmark = pytest.mark.gpu
ADAM_CASES = ("ragged M=35", "ragged M=385", "grid 1x1 M=1")
_runs = {}


class Run:
    """one case on the device: engine, trainer, inputs, and the gradients of one step with injected masks"""

    def __init__(self, name):
        from byolo import Engine
        from byolo.train import HeadTrainer
        c = self.c = G.CASES[name]
        self.name = name
        self.eng = Engine((c.H, c.W, 3), c.cls_cnt, drop_prob=R.DROP_PROB)
        g = self.g = G.build(name, eng=self.eng)
        assert list(self.eng.param_shapes().items()) == list(g.shapes.items())
        self.eng.set_params(R.random_params(g.shapes, R.case_seed(name)))
        self.model = G.Model(self.eng, g, c.aleatoric_loss).finalize()
        self.tr = HeadTrainer(self.model, lr=1e-3, seed=3)
        assert list(self.tr.variables()) == G.head_names(g)[0]
        self.img = torch.from_numpy(np.random.default_rng(R.case_seed(name)).random((c.B, c.H, c.W, 3)).astype(np.float32)).cuda()
        self.boxes, self.labels = G.boxes_for(name)
        self.masks = G.masks_for(name, g) or None
        self.bits = torch.from_numpy(self.eng.pack_masks(self.masks, c.B, 1).view(np.int32)).cuda() if self.masks else None
        self.grads, _, self.losses = self.tr.gradients(self.img, self.boxes, self.labels, mask_bits=self.bits)

    def reference(self, masks, dtype, params=None):
        from byolo import loss as L
        gt = hr.gt_layers(L.encode_gt(self.model.det_layers, self.boxes, self.labels, engine=self.eng))
        p = self.eng.get_params()
        p.update(params or {})
        taps = {k: v.cpu().numpy() for k, v in self.tr.taps().items()}
        return G.reference(self.name, self.g, p, taps, gt, masks, dtype)

    def device(self, grads, losses, acts):
        got = dict(raw=[t.cpu().numpy() for t in self.tr.raw_outputs()], losses=losses, grads=grads)
        if acts:
            got["acts"] = {d["idx"]: self.tr.layer_output(d["idx"]).cpu().numpy() for d in G.head_convs(self.g) if d["op"] == "conv"}
        return got


def _run(name):
    if name not in _runs:
        _runs[name] = Run(name)
    return _runs[name]


@pytest.fixture(scope="module", autouse=True)
def _close_everything():
    yield
    for r in _runs.values():
        r.eng.close()                                           # (closes the trainer first)
    _runs.clear()


def _hold(r, what, grads, losses, masks):
    """every figure printed and recorded, then: nothing beyond its bound"""
    r64, r32 = r.reference(masks, torch.float64), r.reference(masks, torch.float32)
    rr = G.ratios(r.device(grads, losses, acts=masks is not None), r64, r32[0])
    for k, (units, err, ref) in rr.items():
        print("%s | %-44s %8.4f of its bound (max |err| %.3g, max |ref| %.3g)" % (what, k, units, err, ref))
    record_parity("train heads edges: " + what, {k: dict(worst_in_bounds=v[0] if np.isfinite(v[0]) else 1e30, max_abs_err=v[1], max_ref=v[2])
                                                 for k, v in rr.items() if k.startswith("grad ") or k.startswith("raw ")}, kind="train")
    bad = {k: v for k, v in rr.items() if not v[0] <= 1.0}
    assert not bad, (what, bad)


@pytest.mark.parametrize("name", list(G.CASES))
def test_forward_losses_and_gradients(name):
    r = _run(name)
    assert sorted(r.tr.taps()) == sorted({i for d in G.head_convs(r.g) for i, _, _ in d["src"] if i < r.g.first})
    _hold(r, name, r.grads, r.losses, r.masks)


@pytest.mark.parametrize("step", (0, 3))
def test_the_librarys_own_dropout_stream(step):
    """no injected bits: the masks of a step are oracle.rng.keep_mask(seed + step * 0x9E3779B97F4A7C15 mod 2^64, ordinal, shape, p)"""
    from byolo._lib import lib
    r = _run("ragged M=35")
    seed = 0xC0FFEE12345
    r.tr._check(lib.byolo_trainer_set_step(r.tr._tr, step))
    try:
        grads, _, losses = r.tr.gradients(r.img, r.boxes, r.labels, seed=seed)
        assert r.tr.step_count == step
        _hold(r, "ragged M=35, own stream at step %d" % step, grads, losses, G.stream_masks(r.g, seed, step))
    finally:
        r.tr._check(lib.byolo_trainer_set_step(r.tr._tr, 0))


@pytest.mark.parametrize("name", ADAM_CASES)
def test_one_adam_step_and_the_moving_statistics(name):
    """variable sizes such as 40, 21 and 20 x 21 are no multiples of the flat buffer's 64-float segments"""
    r = _run(name)
    tr, names = r.tr, list(r.tr.variables())
    assert any(int(np.prod(s)) % 64 for s in tr.variables().values())
    before = tr.state_dict()
    t = int(before["global_step"]) + 1
    tr.step(r.img, r.boxes, r.labels, mask_bits=r.bits)
    after = tr.state_dict()
    try:
        for n in names:
            g = tr.get(n, "grad").astype(np.float64)
            w, mm, vv = hr.adam(before[n].astype(np.float64), g, before[n + "/Adam"].astype(np.float64),
                                before[n + "/Adam_1"].astype(np.float64), t, tr.lr)
            for got, ref, what in ((after[n], w, "w"), (after[n + "/Adam"], mm, "m"), (after[n + "/Adam_1"], vv, "v")):
                err = np.abs(got - ref)
                assert (err <= 1e-6 * np.maximum(1.0, np.abs(ref))).all(), (n, what, err.max())
        stats = r.reference(r.masks, torch.float64, params={n: before[n] for n in names})[3]
        assert len(stats) == len(tr.moving_statistics()) // 2
        for scope, (mean, var, cnt) in stats.items():
            assert cnt == r.c.expect["M"]
            a, b = "%s/batch_normalization/moving_mean" % scope, "%s/batch_normalization/moving_variance" % scope
            rm, rv = hr.moving((before[a].astype(np.float64), before[b].astype(np.float64)), mean.numpy(), var.numpy(), cnt)
            for got, ref in ((after[a], rm), (after[b], rv)):
                err = np.abs(got - ref)
                assert np.isfinite(got).all() and (err <= 1e-6 * np.maximum(1.0, np.abs(ref))).all(), (scope, err.max())
        assert tr.step_count == t
    finally:
        tr.load_state_dict(before)


def test_determinism_on_three_slices():
    r = _run("ragged M=525")
    assert G.edges(r.g)["a"]["slices"] == 3
    for kw in (dict(mask_bits=r.bits), dict(seed=5)):
        g1, _, l1 = r.tr.gradients(r.img, r.boxes, r.labels, **kw)
        g2, _, l2 = r.tr.gradients(r.img, r.boxes, r.labels, **kw)
        assert l1 == l2
        for n in g1:
            assert np.array_equal(g1[n].view(np.uint32), g2[n].view(np.uint32)), n
    g3, _, _ = r.tr.gradients(r.img, r.boxes, r.labels, mask_bits=r.bits)      # (and the injected masks give the first run's bits again)
    for n in g3:
        assert np.array_equal(g3[n].view(np.uint32), r.grads[n].view(np.uint32)), n


# ---- byolo_trainer_step refuses what it cannot run --------------------------------------------------------------------------------------------
def _refused_at_step(build):
    from byolo import Engine, ByoloError
    from byolo._lib import ERR_ARG
    from byolo.train import HeadTrainer
    eng = Engine((160, 224, 3), 2, drop_prob=R.DROP_PROB)
    g = R.Graph(160, 224, 2, eng=eng)
    R.stem(g, 5, 64)
    g.mark()
    build(g)
    eng.set_params(R.random_params(g.shapes, 1))
    m = G.Model(eng, g, False).finalize()
    tr = HeadTrainer(m)                                         # (making it is fine: the graph is refused when it runs)
    img = torch.rand((2, 160, 224, 3), device="cuda")
    boxes, labels = np.array([[[0.1, 0.1, 0.6, 0.7]]] * 2, np.float32), np.zeros((2, 1), np.int32)
    msgs = []
    for _ in range(2):                                          # the same answer twice: the refusal leaves the trainer in order
        with pytest.raises(ByoloError) as err:
            tr.step(img, boxes, labels)
        assert err.value.code == ERR_ARG
        msgs.append(str(err.value))
    assert msgs[0] == msgs[1] and tr.step_count == 0
    assert np.array_equal(tr.get("det/conv2d/bias"), eng.get_params()["det/conv2d/bias"])      # nothing was updated
    torch.cuda.synchronize()
    eng.close()
    assert not tr._tr
    return msgs[0]


def test_step_refuses_a_concat_of_three_views():
    def build(g):
        g.conv("p", 16, 1)
        g.route("pw", ["p", "w"])
        g.route("pws", ["pw", "s5"])
        g.conv("q", 16, 1)
        g.det("det", 0)
    assert "a concat of more than two views" in _refused_at_step(build)


def test_step_refuses_a_head_convolution_that_reaches_no_loss():
    def build(g):
        g.conv("dangling", 16, 1)
        g.route("back", ["w"])
        g.conv("q", 16, 1)
        g.det("det", 0)
    assert "the output of head layer 'dangling' reaches no loss" in _refused_at_step(build)
