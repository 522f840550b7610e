"""The criterion of tests/test_gpu_layer_f64_fp32.py, E_device <= 4 * unit with unit = max(W, F) on a Winograd layer and F elsewhere
(tests/_layer_ref.py), shown to discriminate -- on the CPU, on every checked layer of every fp32 case (CASES_F32), with the case's own
weights and on inputs of the device's form (plain fp32 values of a post-activation distribution; the stem reads the case's image):

  * every applicable one-line defect of F or W (_layer_ref.MUTANTS_F32: one product dropped, a column that reads zeros for 32 channels
    at one tap, a wrapped column, 32 channels read through their fp16 hi half, one Winograd point dropped for 32 channels, a pad tile
    fed from the neighbour) is at >= 4 x the device bound, i.e. >= 16 * unit; each case records its own smallest ratio, and one test
    over all cases reports the table's minimum and where it occurs;
  * W -- the fp32 Winograd path restated, in both kernels' output orders -- is the layer function: on EVERY Winograd layer of the table
    its distance from layer_eval(float64) is at most 2 x F's on the same layer.  W feeds the device bound through max(W, F), so it
    is held to what an fp32 evaluation of the same function shows (each of W's 16 sums runs over the input channels alone, a ninth of
    F's terms, and nine of them make an output: the same number of roundings as F; measured W / F 0.3 .. 1.3) -- a mis-stated W
    cannot widen a layer's bound beyond 8 F, below every defect above."""
import functools
import os

import pytest

import _layer_ref as R
from conftest import record_parity

MARGIN = 4.0
W_OVER_F = 2.0


def _graph(name):
    H, W, B, T, _, build = R.CASES_F32[name]
    g = R.Graph(H, W, B, T)
    build(g)
    return g


def _synthetic(g, seed):
    """layer index -> a tensor of that layer's shape, values as a leaky activation leaves them in fp32"""
    import torch
    cache = {}

    def fetch(i):
        if i not in cache:
            x = torch.randn(g.tensor_shape(i), generator=torch.Generator().manual_seed(seed + i))
            cache[i] = torch.maximum(x, 0.1 * x)
        return cache[i]
    return fetch


def _setup(name):
    import torch
    torch.set_num_threads(min(os.cpu_count() or 1, 16))
    g = _graph(name)
    seed = R.case_seed(name)
    p = {k: torch.from_numpy(v) for k, v in R.random_params(g.shapes, seed).items()}
    return g, seed, p, _synthetic(g, seed)


@functools.lru_cache(maxsize=None)
def _measured(name):
    """[(layer dict, graph, measure()'s figures with every applicable defect)] of one case: computed once, shared by the tests below"""
    g, seed, p, fetch = _setup(name)
    return [(d, g, R.measure(g, d, p, seed, fetch, mutants=True, precision="f32")) for d in R.checked(g)]


def _ratios(r):
    return {k: v / (MARGIN * r["unit"]) for k, v in r.items() if k.startswith("mutant")}


@pytest.mark.parametrize("name", list(R.CASES_F32))
def test_every_fp32_defect_is_beyond_four_times_the_bound(name):
    table, smallest = {}, (float("inf"), "")
    for d, g, r in _measured(name):
        bound = MARGIN * r["unit"]
        ratios = _ratios(r)
        print("%s / %s (%dx%d/%d %d->%d, %d samples): F %.3g  W %s | defects, in units of the bound: %s"
              % (name, d["name"], d["k"], d["k"], d["stride"], d["Cin"], d["C"], g.samples(d), r["F"], "%.3g (W/F %.2f)" % (r["W"], r["W"] / r["F"]) if "W" in r else "-",
                 "  ".join("%s: %.1f" % (k[7:], v) for k, v in ratios.items())))
        assert ratios, "no defect applies to %s" % d["name"]
        for k, v in ratios.items():
            assert v >= MARGIN, "%s / %s: %s (%s) is only %.2f of the bound" % (name, d["name"], k, R.MUTANTS_F32[int(k[7:])], v)
            table["%s %s" % (d["name"], k)] = dict(worst_in_bounds=v, max_abs_err=r[k], max_ref=bound)
            smallest = min(smallest, (v, "%s, %s" % (d["name"], k)))
        if "W" in r:
            assert r["W"] <= W_OVER_F * r["F"], "%s / %s: W = %.3g is %.2f x F" % (name, d["name"], r["W"], r["W"] / r["F"])
            table[d["name"] + " W / F"] = dict(worst_in_bounds=r["W"] / r["F"], max_abs_err=r["W"], max_ref=r["F"])
    print("%s: smallest defect %.1f x the bound (%s)" % (name, smallest[0], smallest[1]))
    table["smallest of this case"] = dict(worst_in_bounds=smallest[0], max_abs_err=smallest[0], max_ref=1.0)
    record_parity("layer f64 fp32 defects: " + name, table, kind="layers")


def test_the_smallest_defect_ratio_of_the_table():
    """the minimum over every case, layer and defect, and where it occurs (whichever cases ran before: what is missing is computed here)"""
    smallest = min((v, "%s / %s, %s" % (name, d["name"], k)) for name in R.CASES_F32 for d, _, r in _measured(name) for k, v in _ratios(r).items())
    print("smallest defect of the fp32 table: %.1f x the bound (%s)" % smallest)
    record_parity("layer f64 fp32 defects: smallest", {smallest[1]: dict(worst_in_bounds=smallest[0], max_abs_err=smallest[0], max_ref=1.0)}, kind="layers")
    assert smallest[0] >= MARGIN, smallest


@pytest.mark.parametrize("name", ["P1 epilogues wino gemm 5x7x11", "F1 fused N = 64 .. 512 6x10x5", "F1 fused N = 64 .. 512 5x7x11", "W1 wino gemm 128->128 6x10x5"])
def test_the_fp32_winograd_restatement_is_the_layer_function(name):
    """an odd and an even grid, each in wino_output_kernel's AND in wino_fused_kernel's order of the output sums (whichever the case's
    own kernel is); residual and dropout"""
    import torch
    g, seed, p, fetch = _setup(name)
    n = 0
    for d in R.checked(g):
        if not d["check"].get("wino"):
            continue
        src, kw = g.sources(d, fetch, seed), g.spec(d, seed, fetch)
        y64, m = R.layer_eval(src, p, dtype=torch.float64, **kw)
        f = R.distance(R.layer_eval(src, p, dtype=torch.float32, **kw)[0], y64, m)[0]
        for how in ("unfused", "fused"):
            w = R.distance(R.layer_f32(src, p, wino=how, **kw), y64, m)[0]
            print("%s / %s %s: W %.3g  F %.3g  W / F %.2f" % (name, d["name"], how, w, f, w / f))
            assert w <= W_OVER_F * f, (name, d["name"], how, w, f)
            n += 1
        assert torch.equal(R.layer_f32(src, p, **kw), R.layer_eval(src, p, dtype=torch.float32, **kw)[0])      # without `wino`: F itself
    assert n
