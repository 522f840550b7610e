"""The decode stage's float64 comparison, proven on the CPU before the device faces it (tests/_decode_ref.py holds the inputs, the
reference and the mutations; tests/test_decode_f64_gpu.py runs the device through the same `check_rows`).

1. On every input set of the GPU test the float32 and the float64 evaluation of oracle/cpu_ref.py have the same NaN / inf pattern,
   no element lies in a band that a comparison would have to leave out, and the float32 evaluation passes `check_rows` -- with its
   own distance from float64, the floor F(g), below the literal bound 1 in every group (measured: at most 0.11, agree at T = 50; at
   most 0.015 elsewhere), so every allowance the device gets is the literal 1.
2. Each of the ten wrong kernels of `_decode_ref.MUTATIONS` fails `check_rows`; CAUGHT_BY names the sets.
3. `_decode_ref.det_scaled_error` gives the numbers the inline code of tools/soak_decode.py gave before it moved."""
import numpy as np
import pytest

import _decode_ref as R


@pytest.fixture(autouse=True)
def _parity_table_elsewhere(monkeypatch, tmp_path):
    """conftest.record_parity collects DEVICE distances; what these tests compute on the CPU stays out of that table."""
    monkeypatch.setenv("BYOLO_PARITY_TABLE", str(tmp_path / "parity_table.json"))


BUILD = R.build_cases()
STRIDE = R.stride_cases()


def _patterns_bands_floor(c, ref):
    # excluded elements: check_rows has no mask to leave anything out with; what COULD need one are logits inside a band where
    # float32 and float64 disagree about saturation, and elements finite in one reference only
    excluded = R.band_count(c, ref["raw"]) + int((np.isfinite(ref["r32"]) != np.isfinite(ref["r64"])).sum())
    assert excluded == 0
    assert np.array_equal(np.isnan(ref["r32"]), np.isnan(ref["r64"])), "NaN pattern: float32 vs float64 reference"
    assert np.array_equal(np.isinf(ref["r32"]), np.isinf(ref["r64"])), "inf pattern: float32 vs float64 reference"
    inf = np.isinf(ref["r64"])
    assert np.array_equal(ref["r32"][inf], ref["r64"][inf]), "inf signs"
    assert inf.any() and (c.kind == 0 or np.isnan(ref["r64"]).any()), "the plants must saturate something"   # kind 0: no entropies
    # the floor is below the literal bound in every group: allowance(floor) is 1.0 throughout, none is a measurement above 1
    assert R.worst(ref["floor"]) < 1.0, ref["floor"]
    assert ref["floor"].get("ids", {"max_abs_err": 0.0})["max_abs_err"] == 0.0


@pytest.mark.parametrize("c", BUILD, ids=R.case_id)
def test_inputs_need_no_exclusion_and_float32_passes(c):
    ref = R.reference(c)
    _patterns_bands_floor(c, ref)
    R.check_rows(c, R.buffer_with(c, ref["r32"]), ref, "float32 oracle as the device")
    # the right kernel restated in float64 is the float64 reference up to the float32 rounding of the buffer (2^-24 / 1e-4 bounds)
    rr = R.check_rows(c, R.restate(c, ref["raw"]), ref, "float64 restatement as the device")
    assert R.worst(rr["f64"]) <= 2.0 ** -23 / R.RTOL


@pytest.mark.parametrize("c", STRIDE, ids=R.case_id)
def test_grid_stride_inputs_need_no_exclusion(c):
    """The 421 x 419 sets: more lanes than launch_decode_c's largest grid, a plant in the second trip."""
    assert c.B * c.lh * c.lw * 3 > R.STRIDE_LANES
    b, row, col, pr, what = R.plant_lanes(c)[-1]
    assert ((b * c.lh + row) * c.lw + col) * 3 + pr >= R.STRIDE_LANES and what == "-800"
    _patterns_bands_floor(c, R._reference(c))


# Which input sets of the GPU test catch which mutation (every set listed is asserted to fail; `misses` are asserted to pass, so
# that the table stays true).  Measured distances are in profiles/decode_f64.md.
#   * the covariance mutation (swap_triangle) only has to show on spread, where the covariances are O(1): on agree they are about
#     1e-6, below the absolute bound -- there it is the exchanged second MOMENTS (O(1) in both regimes) that the determinant shows,
#     so agree and T = 1 catch it as well;
#   * mi_swapped flips the sign of a mutual information that is O(0.1) on spread, but about 1e-7 on agree (below the absolute
#     bound) and exactly 0 at T = 1: only spread with T = 7 catches it.
CAUGHT_BY = {
    "drop_last_sample": lambda c: True,                             # every kind-2 set with T > 1: spread T = 7, agree T = 50
    "bessel": lambda c: True,
    "swap_col_row": lambda c: True,                                 # all 70 sets, every kind
    "swap_prior_hw": lambda c: True,
    "cell_major": lambda c: True,
    "softmax_minus_one": lambda c: True,                            # every set with C > 1, the capacity boundaries among them
    "entropy_minus_one": lambda c: True,                            # kinds 1 and 2, C > 1
    "swap_triangle": lambda c: True,                                # all 42 kind-2 sets
    "mi_swapped": lambda c: c.regime == "spread" and c.T > 1,       # the 14 spread T = 7 sets; agree and T = 1 cannot see it
    "box_base_plus_one": lambda c: True,
}


@pytest.mark.parametrize("mut", sorted(R.MUTATIONS))
def test_every_mutation_fails_the_assertion(mut):
    caught, wrong = 0, []
    for c in BUILD:
        if not R.applies(mut, c):
            continue
        ref = R.reference(c)
        try:
            R.check_rows(c, R.restate(c, ref["raw"], mut), ref, mut)
            failed = False
        except AssertionError:
            failed = True
        caught += failed
        if failed != CAUGHT_BY[mut](c):
            wrong.append(R.case_id(c))
    assert caught > 0, "%s (%s): no input set of the GPU test notices" % (mut, R.MUTATIONS[mut])
    assert not wrong, "%s: CAUGHT_BY is not what happens on %s" % (mut, wrong)


def test_every_capacity_boundary_catches_the_class_slot_mutations():
    """A slot masked off by one shows at BOTH sides of each capacity boundary, in each kernel (the sets are part of BUILD; this
    spells the claim out)."""
    for mut in ("softmax_minus_one", "entropy_minus_one"):
        for c in BUILD:
            if c.C in R.CAPACITY_C and c.regime == "spread" and R.applies(mut, c):
                ref = R.reference(c)
                with pytest.raises(AssertionError):
                    R.check_rows(c, R.restate(c, ref["raw"], mut), ref, mut)


def test_det_helper_is_the_soaks_inline_code():
    """One seeded case of tools/soak_decode.py's shape (T = 3, logit scale 30: the case its comment cites), the inline code as it
    stood in the soak against the helper that replaced it."""
    g = np.random.default_rng(62)
    B, T, lh, lw, C = 2, 3, 4, 6, 2
    raw = (g.standard_normal((B * T, lh, lw, 3 * 2 * (5 + C))) * 30.0).astype(np.float32)
    c = R.Case(2, C, B, T, lh, lw, "spread", 1, 0, 0, 0)
    import torch
    ref = R.oracle_rows(c, raw, torch.float32)
    got = R.oracle_rows(c, raw, torch.float64).astype(np.float32)
    with np.errstate(all="ignore"):
        raw5d = raw.reshape(B, T, lh, lw, 3, -1)[..., :4].astype(np.float64)
        m2d = (raw5d ** 2).mean(1).transpose(0, 3, 1, 2, 4).reshape(B, -1, 4)
        hb = np.maximum(1.0, np.abs(np.prod(np.abs(ref[..., 4:8].astype(np.float64)) + 16 * 6e-8 * m2d, axis=-1)))
        derr = np.abs(got[..., 12].astype(np.float64) - ref[..., 12]) / hb
    mine = R.det_scaled_error(got, ref, raw, B, T)
    assert mine.shape == derr.shape == (B, 3 * lh * lw) and np.array_equal(mine, derr, equal_nan=True)
    assert np.nanmax(derr) > 0
