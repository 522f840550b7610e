"""The head-training edge cases without a GPU (tests/_head_graphs.py, tests/_heads_ref.py):

  * the bookkeeping of every case -- M, Kc, Kred, N, wgrad slices, mask element counts have the raggedness its comment claims;
  * the bounds the device test applies would catch a one-line defect: the float64 gradients of each case are computed again with each
    defect of _heads_ref.DEFECTS written into the restatement, on synthetic float32 taps, and the defective result must lie at
    >= 4 x the bound of the quantity it shows in (that bound's d32 term measured here, as on the device);
  * the restatement's new arguments leave its defaults bit-identical (the golden fixture);
  * byolo_trainer_create's refusals (host only)."""
import numpy as np
import pytest
import torch

from conftest import golden, golden_params

import _head_graphs as G
import _heads_ref as hr
import _layer_ref as R

MARGIN = 4.0
ADAM_CASES = ("ragged M=35", "ragged M=385", "grid 1x1 M=1")      # the cases whose update the device test checks
_cache = {}


def _case(name):
    if name not in _cache:
        g = G.build(name)
        p = R.random_params(g.shapes, R.case_seed(name))
        taps, gt, masks = G.synthetic_taps(name, g), G.cpu_gt(name, g), G.masks_for(name, g) or None
        r64 = G.reference(name, g, p, taps, gt, masks, torch.float64)
        r32 = G.reference(name, g, p, taps, gt, masks, torch.float32)
        _cache[name] = (g, p, taps, gt, masks, r64, r32)
    return _cache[name]


def _as_run(r):
    return dict(raw=[x.numpy() for x in r[2]], losses=r[1], grads=r[0], acts={k: v.numpy() for k, v in r[4].items()})


def applicable(name, g):
    """the defects whose line of the kernel this case executes"""
    e = G.edges(g)
    grad_in = {n: not all(v["frozen"]) for n, v in e.items()}
    out = [1]
    if any(v["Kc"] % 8 for v in e.values()):
        out.append(2)
    if any(v["Kred"] % 16 for v in e.values()):
        out.append(3)
    if any(v["Kred_dgrad"] % 16 for n, v in e.items() if grad_in[n]):
        out.append(30)
    if any(v["N"] > 128 for v in e.values()):
        out.append(4)
    if any(u and not f for v in e.values() for u, f in zip(v["up"], v["frozen"])):
        out.append(5)
    if any(v["parts"] == 2 and not v["frozen"][1] for v in e.values()):
        out.append(6)
    drops = [int(np.prod(g.tensor_shape(d["idx"]))) for d in g.L[g.first:] if d.get("drop") is not None]
    if len(drops) >= 2 and drops[0] % 32:
        out.append(7)
    if name in ADAM_CASES:
        out.append(8 if e["det"]["M"] > 1 else 9)
    return out


# ---- the edges themselves -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(G.CASES))
def test_each_case_has_the_raggedness_it_claims(name):
    c, g = G.CASES[name], G.build(name)
    e = G.edges(g)
    last = [d for d in G.head_convs(g)][-1]
    assert e[last["name"]]["M"] == c.expect["M"] == c.B * last["H"] * last["W"]
    for key in ("Kc", "N", "slices"):
        for layer, v in c.expect.get(key, {}).items():
            assert e[layer][key] == v, (name, key, layer, e[layer][key])
    drops = [int(np.prod(g.tensor_shape(d["idx"]))) for d in g.L[g.first:] if d.get("drop") is not None]
    assert drops == c.expect.get("masks", [])
    if c.head is G._ragged:
        M = c.expect["M"]
        assert M % 16 and M % 128                               # wgrad's reduction ends inside a BK step; a partial last row tile
        assert [e[n]["Kred"] for n in "abc"] + [e["det"]["Kred"]] == [576, 40, 216, 20] and e["b"]["Kred"] % 16 and e["c"]["Kred"] % 16
        assert e["det"]["Kc"] % 8 == 4 and e["a"]["Kc"] == 4 * 128 + 64 and e["c"]["Kc"] == 128 + 88
        assert [e[n]["Kred_dgrad"] for n in ("b", "c", "det")] == [24, 180, 21] and e["c"]["N"] & 7 and e["det"]["N"] & 7
        assert drops[0] % 32 and drops[1] % 32                  # 32-bit padding between the two dropout layers and behind the second
        # the planner's slices, recomputed from trainer_plan's formula (G.plan_slices spells it out)
        for n, v in e.items():
            assert (v["slices"], v["kslice"], v["last_slice"]) == G.plan_slices(M, v["Kc"], v["N"])
            assert (v["slices"] - 1) * v["kslice"] + v["last_slice"] == M and v["kslice"] % 16 == 0
            if v["slices"] > 1:
                assert v["last_slice"] == c.expect["last_slice"] and v["last_slice"] % 16      # the LAST slice ends inside a BK step
        if M == 35:
            assert G.RED_BLOCKS > M                             # reduction blocks with no row at all
        else:
            assert last["H"] * last["W"] < 128 and M > 3 * 128  # an image boundary inside every row tile, full tiles in front
            assert M % 128 == {385: 1, 525: 13}[M]
    if c.head is G._wide_n:
        assert e["a"]["N"] == 128 + 8
        if c.cls_cnt == 80:
            assert e["det"]["N"] == 128 + 127 and e["det"]["Kred_dgrad"] == 255 and e["det"]["Kred_dgrad"] % 16 == 15
    if c.head is G._wide_c:
        assert e["a"]["N"] > 256 and e["a"]["N"] == 2 * 128 + 8 and e["det"]["Kred"] % 16 == 8
    if c.head is G._views:
        assert (e["a"]["parts"], e["a"]["up"], e["a"]["frozen"]) == (1, [True], [False])
        assert (e["b"]["up"], e["b"]["frozen"]) == ([False, True], [True, False]) and g.by_name["s4"]["C"] == 32      # c_off = 32
        assert (e["c"]["parts"], e["c"]["frozen"]) == (2, [False, False]) and e["c"]["Cin"] == 28 and e["c"]["Kc"] % 16 == 12
        ci, lo = g.by_name["c"]["idx"], g.by_name["lo"]["idx"]
        readers = lambda t: [d["name"] for d in G.head_convs(g) if any(i == t for i, _, _ in d["src"])]
        assert readers(ci) == ["det1", "d", "e"] and e["d"]["parts"] == 1 and e["e"]["parts"] == 2
        assert readers(lo) == ["a", "b"]                          # two scatters into `lo`: the second accumulates
        assert e["det3"]["frozen"] == [True] and e["det3"]["parts"] == 1
        assert e["a"]["slices"] == 2 and e["a"]["last_slice"] % 16
    if name == "grid 1x3":
        assert (last["H"], last["W"]) == (1, 3) and g.by_name["a"]["k"] == 3
    if name == "grid 1x1 M=1":
        assert (last["H"], last["W"], c.B) == (1, 1, 1)


def test_every_defect_is_reached_by_some_case():
    reached = set()
    for name in G.CASES:
        reached.update(applicable(name, G.build(name)))
    assert reached == set(hr.DEFECTS)


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(G.CASES))
def test_explicit_gemms_equal_autograd(name):
    """_heads_ref._Ops with no defect (im2col GEMM, rotated-kernel dgrad, gather / scatter) is the restatement itself"""
    g, p, taps, gt, masks, r64, r32 = _case(name)
    rr = G.ratios(_as_run(G.reference(name, g, p, taps, gt, masks, torch.float64, defect=0)), r64, r32[0])
    assert max(v[0] for v in rr.values()) <= 1e-6, rr


def test_m1_gradients_through_a_batch_norm_are_exactly_the_l2_term():
    g, p, taps, gt, masks, r64, r32 = _case("grid 1x1 M=1")
    for r in (r64, r32):
        for n, v in r[0].items():
            if n.endswith("gamma"):
                assert not v.any(), n
            if n.endswith("kernel") and not n.startswith("det"):
                assert np.array_equal(v, v.dtype.type(hr.L2) * p[n].astype(v.dtype)), n
        for scope, (mean, var, cnt) in r[3].items():
            assert cnt == 1 and not var.numpy().any()


def test_defaults_are_bit_identical_on_the_golden_fixture():
    """old-style calls (no topo / first / names) against the same calls with the defaults spelled out"""
    from oracle import train_ref
    variant = "yolov3_aleatoric"
    fx = golden("fwd_%s.npz" % variant)
    params = golden_params(variant)
    taps = {k: fx["layer_%d" % k].astype(np.float64) for k in (61, 74)}
    taps[36] = fx["layer_36"].astype(np.float64).repeat(2, axis=1).repeat(2, axis=2)        # (stored on a 2x2-strided grid)
    grids = [(taps[k].shape[1], taps[k].shape[2], list(R.PRIORS)) for k in (74, 61, 36)]
    rng = np.random.default_rng(0)
    per_image = [train_ref.encode_boxes(np.array([[0.1, 0.2, 0.6, 0.7], [0.3, 0.1, 0.9, 0.5]]) * s, rng.integers(0, 2, 2), grids, 0.7)
                 for s in (1.0, 0.8)]
    gt = [{k: np.stack([img[l][k] for img in per_image]) for k in per_image[0][l]} for l in range(3)]
    old = hr.grads(params, taps, variant, gt, all_params=params)
    new = hr.grads(params, taps, variant, gt, all_params=params, topo=hr.head_topology(variant, 2), first=75,
                   names=list(hr.trainable_shapes(variant, 2)), drop_prob=0.1, defect=None)
    same = (old[1] == new[1] and all(torch.equal(a, b) for a, b in zip(old[2], new[2])) and list(old[0]) == list(new[0])
            and all(np.array_equal(old[0][n], new[0][n]) for n in old[0]))
    assert same and len(old[0]) == 66


# ---- the defects ---------------------------------------------------------------------------------------------------------------------------
def _moving_ratio(p, stats, defect):
    worst = 0.0
    for scope, (mean, var, cnt) in stats.items():
        mov = tuple(p["%s/batch_normalization/%s" % (scope, n)].astype(np.float64) for n in ("moving_mean", "moving_variance"))
        ref = hr.moving(mov, mean.numpy(), var.numpy(), cnt)[1]
        if defect == 8:
            got = hr.moving(mov, mean.numpy(), var.numpy(), cnt, bessel=False)[1]
        else:
            with np.errstate(divide="ignore", invalid="ignore"):
                vu = var.numpy() * cnt / np.float64(cnt - 1)                      # 0 * 1 / 0
            got = mov[1] - (mov[1] - vu) * (1 - hr.MOMENTUM)
        worst = max(worst, G._ratio(np.abs(got - ref), 1e-6 * np.maximum(1.0, np.abs(ref))))
    return worst


@pytest.mark.parametrize("name", list(G.CASES))
def test_each_defect_lies_beyond_four_times_the_bound(name):
    g, p, taps, gt, masks, r64, r32 = _case(name)
    short = []
    for d in applicable(name, g):
        if d in (8, 9):
            worst, where = _moving_ratio(p, r64[3], d), "moving_variance"
        else:
            rr = G.ratios(_as_run(G.reference(name, g, p, taps, gt, masks, torch.float64, defect=d)), r64, r32[0])
            if name not in G.DROPOUT_CASES:                  # (the device test holds the activations of the dropout cases only)
                rr = {k: v for k, v in rr.items() if not k.startswith("activation")}
            where = max(rr, key=lambda k: rr[k][0])
            worst = rr[where][0]
        print("%-22s defect %2d (%s): %.3g x the bound, in %s" % (name, d, hr.DEFECTS[d], worst, where))
        if not worst >= MARGIN:
            short.append((d, worst, where))
    assert not short, (name, short)


# ---- byolo_trainer_create refuses what it cannot train (host only) ---------------------------------------------------------------------------
def _refused(build, aleatoric_loss=False):
    from byolo import Engine, ByoloError
    from byolo.train import HeadTrainer
    eng = Engine((160, 224, 3), 2, drop_prob=R.DROP_PROB)
    g = R.Graph(160, 224, 2, 3, eng=eng)
    build(g)
    with pytest.raises(ByoloError) as err:
        HeadTrainer(G.Model(eng, g, aleatoric_loss))
    assert not len(eng._trainers)                               # nothing half-made is left bound to the handle
    eng.close()
    return str(err.value)


def test_create_refuses_a_stride_2_head_convolution():
    def build(g):
        R.stem(g, 4, 64)
        g.mark()
        g.conv("down", 32, 3, 2)
        g.det("det", 0)
    assert "head layer 'down'" in _refused(build)


def test_create_refuses_a_residual_in_the_head():
    def build(g):
        R.stem(g, 5, 64)
        g.mark()
        g.conv("p", 64, 1)
        g.conv("q", 64, 3, res="p")
        g.det("det", 0)
        build.at = g.by_name["q"]["idx"]
    msg = _refused(build)
    assert "head layer %d" % build.at in msg and "only convolution, route, upsample and detection layers train" in msg


def test_create_refuses_a_t_stacked_head_layer():
    def build(g):
        R.stem(g, 5, 64)
        g.stack("st", "w")
        g.mark()
        g.conv("r", 32, 1, drop=True)
        g.det("det", 2)
    assert "head layer 'r' is T-stacked" in _refused(build)


def test_create_refuses_a_graph_with_no_detection_layer_after_the_mark():
    def build(g):
        R.stem(g, 5, 64)
        g.det("det", 0)
        g.mark()
        g.route("back", ["w"])
        g.conv("p", 32, 1)
    assert "no detection layer after byolo_mark_backbone_end" in _refused(build)


def test_a_valid_graph_is_accepted_after_a_refusal():
    """the same process makes a trainer for every case's graph (host only): variables in creation order, closed with its engine"""
    from byolo import Engine
    from byolo.train import HeadTrainer
    for name, c in G.CASES.items():
        eng = Engine((c.H, c.W, 3), c.cls_cnt, drop_prob=R.DROP_PROB)
        g = G.build(name, eng=eng)
        assert list(eng.param_shapes().items()) == list(g.shapes.items())
        tr = HeadTrainer(G.Model(eng, g, c.aleatoric_loss))
        assert list(tr.variables()) == G.head_names(g)[0] and sorted(tr.moving_statistics()) == sorted(G.head_names(g)[1])
        layout, _ = eng.mask_layout(c.B, 1)
        assert [n for _, n in layout] == c.expect.get("masks", [])
        if len(layout) == 2:
            assert layout[1][0] == -(-layout[0][1] // 32) * 32 != layout[0][1]      # the second layer starts at the PADDED offset
        eng.close()
        assert not tr._tr
