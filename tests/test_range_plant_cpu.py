"""The inputs of tests/test_gpu_range_flag.py shown good on the CPU (tests/_range_plant.py), on every checked convolution of every distinct
graph of the layer suite and of every case the device test runs, on the oracle's own float64 forward of the case:

  * the helper finds the plantings A and B, and the input condition holds: the boundary 16380 is >= 8 bounds (4 * max(S, F) * m, under
    the planted parameters) from the top and from the second element;
  * above: exactly ONE element of the layer is >= 16380, in float64 and in float32, and in the emulated split-f16 arithmetic exactly
    that element's hi half is inf;  below: none is, the emulation is finite everywhere and within 4 * max(S, F) of float64 -- so the
    emulation itself rounds the band 4 v in [65504, 65520) DOWN to 65504, as v_cvt_pk_f16_f32 must;
  * the downstream condition of `below` -- every other split-stored tensor of the graph below 16380 / 2 under the planted parameters,
    walked in float64 by oracle/cpu_ref.py -- holds for the A of the layers marked 'together', and CANNOT hold for the others: a layer
    a later residual adds hands its lifted channel to that sum (_range_plant.feeds_a_sum), and two or more He-scaled convolutions
    behind a channel of 16380 carry it beyond 8190 for every qualifying channel tried.  The test asserts which of the two it is; the
    device test plants the first kind at once and expects clean status words, the second kind alone and expects that the layer
    reported is not the planted one;
  * three deliberately wrong detectors, applied to the same reference tensors, each misjudge a planting, named in the output: vmax
    taken before the residual add, the threshold held against the value instead of 4 * value, and > 65504 for >= 65520.

The device test asserts the same conditions on the device's own inputs; this file is what makes them known good beforehand."""
import functools
import os

import pytest
import torch

import _layer_ref as R
import _range_plant as P
from conftest import record_parity
from test_layer_ref_cpu import _DISTINCT, _graph

NAMES = _DISTINCT + [n for n in P.DEVICE_CASES if n not in _DISTINCT]


def plan_case(name, seed):
    """[(layer, kind, setting, judge()'s dict, the residual the layer adds or None, A meets the downstream condition)] of one case"""
    torch.set_num_threads(min(os.cpu_count() or 1, 16))
    g = _graph(name)
    p = {k: torch.from_numpy(v) for k, v in R.random_params(g.shapes, seed).items()}
    outs = P.walk(g, p, seed)
    fetch = lambda i: outs[i]
    found = []
    for d in R.checked(g):
        if d["det"]:
            continue
        log = []
        ok = lambda q, d=d: P.others_in_half_range(g, P.walk(g, q, seed), [d])[0]
        got = {} if P.feeds_a_sum(g, d) else P.choose(g, d, p, seed, fetch, kinds=("A",), downstream=ok, log=log)
        together = "A" in got
        if not together:
            got = P.choose(g, d, p, seed, fetch, kinds=("A",), log=log)
        got.update(P.choose(g, d, p, seed, fetch, kinds=("B",), log=log))
        assert "A" in got and "B" in got, "%s / %s: no channel qualifies (%s): change the case's seed for this suite: %s" % (name, d["name"], sorted(got), "; ".join(log))
        for kind in ("A", "B"):
            if kind == "B" and got["B"]["above"]["c"] == got["A"]["above"]["c"]:
                continue
            for setting in ("above", "below"):
                found.append((d, kind, setting, got[kind][setting], g.spec(d, seed, fetch)["residual"], together))
    return g, seed, fetch, found


@functools.lru_cache(maxsize=None)
def _plantings(name):
    """computed once per case, read by both tests"""
    return plan_case(name, P.plant_seed(name))


@pytest.mark.parametrize("name", NAMES)
def test_the_plantings_straddle_the_boundary_by_eight_bounds(name):
    g, seed, fetch, found = _plantings(name)
    table = {}
    for d, kind, setting, r, _, together in found:
        print("%s / %s %s %s: channel %d beta %.9g | top %.9g at %s (row %d)  second %.9g  bound %.3g  gap / 2 = %.1f bounds | S %.3g F %.3g"
              % (name, d["name"], kind, setting, r["c"], r["beta"], r["top"], r["at"], r["row"], r["second"], r["bound"],
                 (r["top"] - r["second"]) / 2 / r["bound"], r["S"], r["F"]))
        assert r["ok"], (name, d["name"], kind, setting, r["why"])
        assert (r["top"] - r["second"]) / 2 >= P.GUARD * r["bound"]
        src, kw = g.sources(d, fetch, seed), g.spec(d, seed, fetch)
        y64 = r["y64"]
        y32 = R.layer_eval(src, r["p"], dtype=torch.float32, **kw)[0]
        wino, direct = "wino" in d["check"], dict(direct=True) if g.direct(d) else {}
        hi, lo = R.layer_split(src, r["p"], wino=wino, halves=True, **direct, **kw)
        if setting == "above":
            for y in (y64, y32):
                out = (y.abs() >= P.LIMIT).nonzero().tolist()
                assert out == [list(r["at"])], (name, d["name"], kind, out, r["at"])
            assert torch.isinf(hi).nonzero().tolist() == [list(r["at"])] and not bool(torch.isnan(hi).any())
            assert P.flags(y64) and P.flags(y32)
        else:
            assert not bool((y64.abs() >= P.LIMIT).any()) and not bool((y32.abs() >= P.LIMIT).any())
            assert bool(torch.isfinite(hi).all()) and bool(torch.isfinite(lo).all())
            E, _ = R.distance(hi + lo, y64, r["m"])
            assert E <= P.MARGIN * r["unit"], (name, d["name"], kind, E, r["unit"])
            assert float(hi[r["at"]]) * R.ACT_SCALE == 65504.0 and P.LIMIT - r["top"] < 4.0      # the band below the boundary, rounded down
            assert not P.flags(y64) and not P.flags(y32)
            if kind == "A":
                inside, worst = P.others_in_half_range(g, P.walk(g, r["p"], seed), [d])
                print("    %s: every other split-stored tensor |v| <= %.6g%s" % ("together" if together else "alone", worst,
                      " (a later residual adds this layer)" if P.feeds_a_sum(g, d) else ""))
                assert inside == together, (name, d["name"], worst)
                assert not (together and P.feeds_a_sum(g, d))
        table["%s %s %s" % (d["name"], kind, setting)] = dict(worst_in_bounds=(r["top"] - r["second"]) / 2 / r["bound"], max_abs_err=r["bound"], max_ref=r["top"])
    record_parity("range plant: " + name, table, kind="layers")


# residual layers of both kinds of epilogue (direct and Winograd), and of the direct small-Cin kernel
@pytest.mark.parametrize("names", [("A4 kx3 epilogues 5x7x11", "C4 wino epilogues 3x5x23", "K direct small-Cin 5x7x3")])
def test_each_wrong_detector_misjudges_a_named_planting(names):
    caught = {w: [] for w in P.WRONG}
    for name in names:
        _, _, _, found = _plantings(name)
        for d, kind, setting, r, residual, _ in found:
            want = setting == "above"
            assert P.flags(r["y64"], residual) == want
            for w in P.WRONG:
                if w == "before the residual" and residual is None:
                    continue
                if P.flags(r["y64"], residual, detector=w) != want:
                    caught[w].append("%s / %s %s %s" % (name, d["name"], kind, setting))
    for w in P.WRONG:
        print("detector '%s' is wrong on %d plantings: %s" % (w, len(caught[w]), "; ".join(caught[w][:6])))
        assert caught[w], "no planting tells the detector '%s' from the right one" % w
