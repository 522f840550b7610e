"""ONE activation of ONE layer moved across the split-f16 range (|value| < 65520 / 4 = 16380, include/byolo.h BYOLO_PREC_SPLIT_F16), for
tests/test_range_plant_cpu.py and tests/test_gpu_range_flag.py.

A planting changes beta[c] of one channel of one checked layer d (tests/_layer_ref.py) and nothing else: the folded shift moves, the
packed weights and every tensor in front of d keep their bits.  Lifted by ~16380 the whole channel is on the linear side of the leaky
activation, so with  t = y - beta  (float64, dropout and residual included, independent of beta) and t1 >= t2 its two largest values

    above:  beta = 16380 - (t1 + t2) / 2         top and second straddle the boundary at equal distances: ONE element is out of range
    below:  beta = 16380 - (t1 - t2) / 2 - t1    top = 16380 - (top - second) / 2: nothing is out of range, and 4 * top sits in the
                                                 band [65504, 65520) where the hi half must round DOWN to 65504

beta is an fp32 parameter (one ulp at 16380 is 1e-3), so everything is judged on the layer evaluated again under the beta that was
actually stored.  Condition on the inputs, not a measurement: with  bound = 4 * unit * m  at the top and at the second element -- unit =
max(S, F) of _layer_ref.measure() under the planted parameters, the criterion every kernel is held to by tests/test_gpu_layer_f64.py --
the boundary is >= 8 bounds away from both (and so is half their gap).  A kernel anywhere inside its bound is then at most one eighth
of the way to the boundary: the flag the device must raise is decided by the float64 reference alone.  8: three binary orders over the
kernel's own allowance, none of them measured on a kernel.  (The unit of an `above` planting is measured on the same channel one gap
lower, i.e. under its `below` planting: the emulation S holds an inf above, by design.)

Channel choice.  A: among the channels that qualify, the one whose top element has the largest row index (s * H + y) * W + x -- the last
row tile / Winograd unit, partial on these graphs.  B: the qualifying channel with the largest index -- the last column tile / 4-channel
group.  edge: the best qualifying channel whose top lies in the last row or column of an odd grid (a Winograd tile that stores one to
three of its four outputs).  For `below` a channel must also leave every OTHER split-stored tensor of the graph below 16380 / 2 (walk())."""
import numpy as np
import torch

import _layer_ref as R

LIMIT = 65520.0 / R.ACT_SCALE      # 16380: the smallest magnitude whose hi half rounds to infinity
GUARD = 8.0
MARGIN = 4.0                       # the layer suites' criterion: E <= 4 * unit
LIFT = 16384.0                     # any beta that clears the leaky kink; a power of two: y - LIFT is exact to 2e-12 in float64
WALKS = 8                          # ... of them walked through the whole graph (the downstream condition of `below`)
TRIES = 24                         # candidates judged in full per choice (the cheap estimate in front of it sorts out most)


# the cases of tests/test_gpu_range_flag.py that run the whole procedure (sites 1, 2, 6, 7, 8, 9 of profiles/range_flag.md)
DEVICE_CASES = ["A4 kx3 epilogues 5x7x11", "B1 p1 5x7x11", "B3 p1 ksplit=3 5x7x11", "B2 general 12x20x7", "B2 general 10x14x7",
                "B3 every loop streamk=2 6x10x5", "B3 every loop ksplit=3 6x10x5", "A2 kx3 128x256 3x5x20", "D2 stacked T=3 5x7x4",
                "C1 wino<256> 256->256 3x5x23", "C2 wino<128> 3x5x23", "C3 wino chunks 5x7x11", "C4 wino epilogues 3x5x23",
                "D2 stacked T=3 wino 5x7x4", "K direct small-Cin 5x7x3", "K direct small-Cin 6x10x2"]
# A case on whose own seed some checked layer has no channel with a gap of 16 bounds between its two largest values (a few hundred to
# a few hundred thousand order-one values per channel against a bound of 0.02 .. 0.03) draws its parameters, image and masks for this
# suite from another seed: the first k >= 1 of  case_seed(name + " | range k")  on which every layer has one.
RESEED = {"C5 wino 1x3x9": 1, "B1 p1 5x7x11": 1, "K direct small-Cin 6x10x2": 1, "B3 every loop ksplit=3 6x10x5": 2}


def plant_seed(name):
    return R.case_seed(name if name not in RESEED else "%s | range %d" % (name, RESEED[name]))


def beta_name(d):
    return d["name"] + "/batch_normalization/beta"


def with_beta(p, d, c, value):
    """p (name -> fp32 torch tensor) with beta[c] of layer d replaced; every other tensor shared, p itself untouched"""
    q = dict(p)
    b = p[beta_name(d)].clone()
    b[c] = float(np.float32(value))
    q[beta_name(d)] = b
    return q


def _eval64(g, d, p, seed, fetch):
    return R.layer_eval(g.sources(d, fetch, seed), p, dtype=torch.float64, **g.spec(d, seed, fetch))


def free_part(g, d, p, seed, fetch):
    """(t, m): the layer's float64 output minus beta with every channel lifted clear of the kink, and the magnitude m at that lift"""
    q = dict(p)
    q[beta_name(d)] = torch.full_like(p[beta_name(d)], LIFT)
    y, m = _eval64(g, d, q, seed, fetch)
    return y - LIFT, m


def beta_for(t1, t2, setting):
    return LIMIT - (t1 + t2) / 2 if setting == "above" else LIMIT - (t1 - t2) / 2 - t1


def top_two(y):
    """((value, (s, y, x, c)) of the largest, of the second largest) element of a whole tensor"""
    v, i = y.flatten().topk(2)
    at = [tuple(int(k) for k in np.unravel_index(int(j), tuple(y.shape))) for j in i]
    return (float(v[0]), at[0]), (float(v[1]), at[1])


def judge(g, d, p, seed, fetch, c, setting, t1, t2):
    """Plant (c, setting) and evaluate the layer again under the stored beta: a dict with the planted parameters `p`, top / second /
    bound / unit, where the top element lies, and `ok` -- the input condition (with `why` where it fails)."""
    q = with_beta(p, d, c, beta_for(t1, t2, setting))
    y64, m = _eval64(g, d, q, seed, fetch)
    (top, at), (second, at2) = top_two(y64)
    # (above: the emulation S holds an inf there by design, so the unit is that of the SAME channel one gap lower -- the `below`
    #  planting, beta smaller by t1 - t2 --, where every value is finite and every rounding has the same size)
    r = R.measure(g, d, q if setting == "below" else with_beta(p, d, c, beta_for(t1, t2, "below")), seed, fetch)
    bound = MARGIN * r["unit"] * max(float(m[at]), float(m[at2]))
    out = dict(p=q, c=c, setting=setting, beta=float(q[beta_name(d)][c]), top=top, second=second, at=at, at2=at2, bound=bound, unit=r["unit"],
               S=r["S"], F=r["F"], row=(at[0] * d["H"] + at[1]) * d["W"] + at[2], n_out=int((y64.abs() >= LIMIT).sum()), y64=y64, m=m)
    why = []
    if at[3] != c or at2[3] != c:
        why.append("top / second lie in channels %d / %d" % (at[3], at2[3]))
    if not (top - second) / 2 >= GUARD * bound:
        why.append("half the gap %.3g is below 8 bounds of %.3g" % ((top - second) / 2, bound))
    if setting == "above" and not (top - LIMIT >= GUARD * bound and LIMIT - second >= GUARD * bound and out["n_out"] == 1):
        why.append("top %.9g / second %.9g do not straddle 16380 by 8 bounds of %.3g" % (top, second, bound))
    if setting == "below" and not (LIMIT - top >= GUARD * bound and out["n_out"] == 0):
        why.append("top %.9g is not 8 bounds of %.3g below 16380" % (top, bound))
    out["ok"], out["why"] = not why, "; ".join(why)
    return out


def choose(g, d, p, seed, fetch, kinds=("A", "B"), settings=("above", "below"), downstream=None, log=None):
    """{kind: {setting: judge()'s dict}} for layer d on the input fetch() hands out.  kinds: 'A' | 'B' | 'edge' (above).  downstream:
    planted parameters -> bool, asked for the `below` planting (walk()).  A kind no channel qualifies for is missing from the result."""
    t, m = free_part(g, d, p, seed, fetch)
    C = t.shape[3]
    v, i = t.reshape(-1, C).topk(2, dim=0)
    t1, t2, row = v[0], v[1], i[0]
    unit0 = max(R.measure(g, d, p, seed, fetch)["unit"], 2.0 ** -23)       # (2^-23: hi + lo of a value holds 22 bits)
    est = MARGIN * unit0 * m.reshape(-1, C).gather(0, i).amax(dim=0)       # the bound, estimated: only sorts candidates out early
    likely = [c for c in range(C) if float(t1[c] - t2[c]) / 2 >= GUARD * float(est[c])]
    yy, xx = (row // d["W"]) % d["H"], row % d["W"]
    order = {"A": sorted(likely, key=lambda c: (-int(row[c]), -c)), "B": sorted(likely, key=lambda c: -c),
             "edge": sorted([c for c in likely if int(yy[c]) == d["H"] - 1 or int(xx[c]) == d["W"] - 1], key=lambda c: (-int(row[c]), -c))}
    judged, out = {}, {}
    if log is not None:
        log.append("%d of %d channels likely (unit %.3g, largest gap %.3g, bound estimated %.3g .. %.3g)"
                   % (len(likely), C, unit0, float((t1 - t2).max()), float(est.min()), float(est.max())))
    for kind in kinds:
        for c in order[kind][:TRIES if downstream is None else WALKS]:
            if c not in judged:
                res = {s: judge(g, d, p, seed, fetch, c, s, float(t1[c]), float(t2[c])) for s in settings}
                good = all(r["ok"] for r in res.values())
                if good and downstream is not None and "below" in res:
                    good = downstream(res["below"]["p"])
                    if not good and log is not None:
                        log.append("channel %d: another tensor leaves half the range" % c)
                elif log is not None:
                    log.append("channel %d: %s" % (c, " | ".join(r["why"] for r in res.values() if r["why"])))
                judged[c] = res if good else None
            if judged[c] is not None:
                out[kind] = judged[c]
                break
    return out


def walk(g, p, seed):
    """oracle/cpu_ref.py's forward of the graph in float64 under the parameters p: layer index -> tensor"""
    from oracle import cpu_ref
    p64 = {k: v.double() for k, v in p.items()}
    img = np.random.default_rng(seed).random((g.B, g.H, g.W, 3)).astype(np.float32)
    saved = cpu_ref.topology
    cpu_ref.topology = lambda *a, **k: g.topology()
    try:
        with torch.no_grad():
            return cpu_ref.forward(p64, img, "yolov3", T=g.T, seed=seed, drop_prob=R.DROP_PROB, dtype=torch.float64, taps="all")["layers"]
    finally:
        cpu_ref.topology = saved


def stored(g):
    """the layers whose output is a split-stored tensor: every convolution and every residual sum (a detection head's raw output is
    fp32; route / upsample / stack are views)"""
    return [l for l in g.L if l["op"] in ("conv", "res")]


def feeds_a_sum(g, d):
    """layer d's output is the shortcut operand of a later residual add: that sum holds the lifted channel plus a leaky activation
    (>= -0.1 |.|), so no `below` planting of d can leave it below 16380 / 2 -- the downstream condition cannot be met for d, whatever
    the channel and the seed.  Such a layer's `below` planting is judged on the layer alone, and the device test runs it by itself:
    the first layer reported must not be d (status words take the SMALLEST flagged index, and nothing in front of d changed)."""
    return any(l["op"] == "res" and l["shortcut"] == d["out"] for l in g.L)


def others_in_half_range(g, outs, planted):
    """every split-stored tensor except those of the planted layers (their convolution and the sum it owns) stays below 16380 / 2"""
    skip = {i for d in planted for i in (d["idx"], d["out"])}
    worst = max([float(outs[l["idx"]].abs().max()) for l in stored(g) if l["idx"] not in skip] or [0.0])
    return worst < LIMIT / 2, worst


# ---- the detector, and three wrong ones (tests/test_range_plant_cpu.py) ---------------------------------------------------------
def flags(y, residual=None, detector="right"):
    """Would a kernel's  vmax >= 65520  raise on the layer output y (fp32 or float64; residual: the tensor the epilogue added)?"""
    s = y * R.ACT_SCALE                                    # what the kernel holds: the pre-scaled value
    if detector == "right":
        return bool((s.abs() >= 65520.0).any())
    if detector == "before the residual":                  # vmax taken before the add
        return bool(((y - residual.to(y.dtype)) * R.ACT_SCALE).abs().ge(65520.0).any())
    if detector == "value, not 4 * value":                 # the threshold off by ACT_SCALE
        return bool((y.abs() >= 65520.0).any())
    if detector == "> 65504":                              # the largest finite fp16 taken for the boundary
        return bool((s.abs() > 65504.0).any())
    raise KeyError(detector)


WRONG = ("before the residual", "value, not 4 * value", "> 65504")
