"""The criterion of tests/test_gpu_layer_f64.py, E_device <= 4 * max(E_S, E_F) (tests/_layer_ref.py), shown to discriminate -- on the CPU,
on every checked layer of every case of the device test, with the case's own weights and on inputs of the device's form (hi + lo pairs
of a post-activation distribution):

  * the correct emulation S holds it trivially; S / F is printed (the emulated split-f16 arithmetic against plain float32);
  * every applicable one-line defect of S (_layer_ref.MUTANTS: a lost lo_w / lo_x term in one 32-channel chunk, a wrapped column, a
    residual from its hi half, a lost lo plane of V, a pad tile fed from the neighbour) is at >= 4 x the bound, i.e. >= 16 * max(S, F) --
    the device test cannot hide such a defect behind its margin;
  * the float64 single-layer evaluation is oracle/cpu_ref.py's own layer: the oracle's forward() walks the case's graph in float64 and
    every checked layer, evaluated alone on the oracle's input of it, equals the oracle's output to 1e-12.

The ratios go to record_parity, into the table the device test writes its {E, S, F} to (profiles/layer_f64.md quotes both)."""
import os

import pytest

import _layer_ref as R
from conftest import record_parity

MARGIN = 4.0


def _graph(name):
    H, W, B, T, _, build = R.CASES[name]
    g = R.Graph(H, W, B, T)
    build(g)
    return g


def _synthetic(g, seed):
    """layer index -> a tensor of that layer's shape, values as a leaky activation leaves them, exactly representable as hi + lo"""
    import torch
    cache = {}

    def fetch(i):
        if i not in cache:
            x = torch.randn(g.tensor_shape(i), generator=torch.Generator().manual_seed(seed + i))
            hi, lo = R._split(torch.maximum(x, 0.1 * x), R.ACT_SCALE)
            cache[i] = hi + lo
        return cache[i]
    return fetch


# distinct graphs only (the same graph under other plan options has the same layers)
_DISTINCT = list({R.CASES[n][:4] + (R.CASES[n][5],): n for n in reversed(list(R.CASES))}.values())[::-1]


@pytest.mark.parametrize("name", _DISTINCT)
def test_every_mutant_is_beyond_four_times_the_bound(name):
    import torch
    torch.set_num_threads(min(os.cpu_count() or 1, 16))
    g = _graph(name)
    seed = R.case_seed(name)
    p = {k: torch.from_numpy(v) for k, v in R.random_params(g.shapes, seed).items()}
    fetch = _synthetic(g, seed)
    table = {}
    for d in R.checked(g):
        r = R.measure(g, d, p, seed, fetch, mutants=True)
        bound = MARGIN * max(r["S"], r["F"])
        ratios = {k: v / bound for k, v in r.items() if k.startswith("mutant")}
        print("%s / %s (%dx%d %d->%d, %d samples): F %.3g  S %.3g  S/F %.2f | mutants, in units of the bound: %s"
              % (name, d["name"], d["k"], d["k"], d["Cin"], d["C"], g.samples(d), r["F"], r["S"], r["S"] / r["F"],
                 "  ".join("%s: %.1f" % (k[7:], v) for k, v in ratios.items())))
        assert r["S"] <= bound
        assert ratios, "no mutant applies to %s" % d["name"]
        for k, v in ratios.items():
            assert v >= MARGIN, "%s / %s: %s (%s) is only %.2f of the bound" % (name, d["name"], k, R.MUTANTS[int(k[7:])], v)
        for k, v in ratios.items():                        # in units of the bound; beside them S / F, in units of F
            table["%s %s" % (d["name"], k)] = dict(worst_in_bounds=v, max_abs_err=r[k], max_ref=bound)
        table[d["name"] + " S / F"] = dict(worst_in_bounds=r["S"] / r["F"], max_abs_err=r["S"], max_ref=r["F"])
    record_parity("layer f64 mutants: " + name, table, kind="layers")


@pytest.mark.parametrize("name", ["A4 kx3 epilogues 5x7x11", "B1 p1 5x7x11", "B2 general 12x20x7", "D2 stacked T=3 5x7x4"])
def test_the_single_layer_evaluation_is_the_oracles_layer(name, monkeypatch):
    """residual, dropout, detection bias | 1x1 | stride 2, upsampled two-source concat | dropout of a replayed and of a stacked layer"""
    import numpy as np
    import torch
    from oracle import cpu_ref
    g = _graph(name)
    seed = R.case_seed(name)
    p = {k: torch.from_numpy(v).double() for k, v in R.random_params(g.shapes, seed).items()}
    img = np.random.default_rng(seed).random((g.B, g.H, g.W, 3)).astype(np.float32)
    monkeypatch.setattr(cpu_ref, "topology", lambda *a, **k: g.topology())
    with torch.no_grad():
        outs = cpu_ref.forward(p, img, "yolov3", T=g.T, seed=seed, drop_prob=R.DROP_PROB, dtype=torch.float64, taps="all")["layers"]
    for d in R.checked(g):
        fetch = lambda i: outs[i]
        y64, m = R.layer_eval(g.sources(d, fetch), p, dtype=torch.float64, **g.spec(d, seed, fetch))
        ref = outs[d["out"]]
        assert y64.shape == ref.shape
        err = float(((y64 - ref).abs() / ref.abs().clamp(min=1.0)).max())
        assert err <= 1e-12, (name, d["name"], err)
        assert bool((m >= y64.abs() * (1 - 1e-12)).all())                 # m bounds the layer's value: an error relative to m is <= one relative to |y|
