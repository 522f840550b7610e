"""The localisation part of the evaluation without a GPU: the numpy restatement (tests/_eval_loc_ref.py) on planted data, the
product's host-side reduction (byolo/eval_loc.py) against it, the quantile literals, auroc_fp on hand cases, the inversion of a
planted decode, and the argument checks of byolo_eval_set_loc."""
import ctypes
import math
import os
import re
import statistics

import numpy as np
import pytest

import _eval_loc_ref as lr
import _eval_ref as er
from conftest import REPO

f32, f64 = np.float32, np.float64
N = 20000
SEED = 11


def _planted():
    rng = np.random.default_rng(SEED)
    var = rng.uniform(0.01, 0.5, (4, N))
    r = rng.normal(0.0, 1.0, (4, N)) * np.sqrt(var)
    return r, var


def test_planted_residuals_are_calibrated():
    """r ~ N(0, var), 20 000 true positives per coordinate: every coverage level within four binomial standard deviations of P,
    mean z^2 within four standard deviations (var z^2 = 2) of 1; with all variances quartered sigma_scale is 2 by the same
    margin."""
    from byolo import eval_loc
    r, var = _planted()
    for k in range(4):
        for impl in (lr.coord_stats, eval_loc.coord_stats):
            s = impl(r[k], var[k])
            assert s['n'] == N and s['n_bad_var'] == 0
            for P, c in zip(lr.LEVELS, s['coverage']['count']):
                assert abs(c / N - P) <= 4 * math.sqrt(P * (1 - P) / N), (k, P, c / N)
            assert abs(s['mean_z2'] - 1) <= 4 * math.sqrt(2 / N), (k, s['mean_z2'])
            assert s['coverage']['miscalibration_area'] <= 4 * math.sqrt(0.25 / N)
            assert s['ence'] <= 0.05                                           # five bins of 4000: sqrt(mean r^2) within a few per cent of sigma
            q = impl(r[k], var[k] / 4)
            assert abs(q['sigma_scale'] - 2) <= 4 * math.sqrt(2 / N), (k, q['sigma_scale'])
            assert q['coverage']['count'][8] / N < 0.65                        # |z| <= 1.645 at twice the spread: 59 %


def _close(got, exp, n, scale):
    if exp != exp:
        return got != got
    return abs(got - exp) <= max(n, 1) * 2.0 ** -52 * scale


def check_stats(got, exp, what=''):
    """got: the product's dict of one kind and coordinate; exp: lr.coord_stats.  Integers exactly, means within the error of a
    float64 sum of n terms (n 2^-52 mean|x|, the rule of tests/test_eval_gpu.py)."""
    n = exp['n']
    for k in ('n', 'n_bad_var', 'n_outside'):
        assert got[k] == exp[k], (what, k, got[k], exp[k])
    assert got['coverage']['count'] == exp['coverage']['count'] and got['coverage']['levels'] == exp['coverage']['levels'], what
    for k in ('mean_err', 'mean_var', 'mean_z2', 'nll'):
        assert _close(got[k], exp[k], n, exp['_abs'][k]), (what, k, got[k], exp[k])
    if n:
        # a square root halves a relative error
        assert _close(got['rmse'], exp['rmse'], n, exp['rmse']) and _close(got['sigma_scale'], exp['sigma_scale'], n, exp['sigma_scale']), what
        assert _close(got['coverage']['miscalibration_area'], exp['coverage']['miscalibration_area'], 11, 1.0), what
    else:
        assert all(math.isnan(got[k]) for k in ('rmse', 'sigma_scale', 'ence')) and math.isnan(got['coverage']['miscalibration_area'])
    rel = 0.0
    for g, e in zip(got['sigma_bins'], exp['sigma_bins']):
        assert g['n'] == e['n'], what
        assert _close(g['mean_var'], e['mean_var'], e['n'], e['mean_var']) and _close(g['mean_r2'], e['mean_r2'], e['n'], e['mean_r2']), (what, g, e)
        if e['n'] and e['mean_var'] > 0:
            rel = max(rel, math.sqrt(e['mean_r2'] / e['mean_var']))
    if n:
        # each term |1 - sqrt(mean_r2 / mean_var)| errs by at most n 2^-52 (1 + sqrt(mean_r2 / mean_var))
        assert _close(got['ence'], exp['ence'], n, 1.0 + rel), (what, got['ence'], exp['ence'])


def check_class_stats(got, exp, what=''):
    assert got['n'] == exp['n'], what
    for k in ('mean_z2', 'nll'):
        assert _close(got[k], exp[k], exp['n'], exp['_abs'][k]), (what, k, got[k], exp[k])


def test_product_reduction_equals_the_restatement():
    from byolo import eval_loc
    rng = np.random.default_rng(3)
    for n in (0, 1, 4, 7, 203):
        var = rng.uniform(0.01, 0.5, n)
        r = rng.normal(0, 1, n) * np.sqrt(var) * 1.3
        if n >= 7:
            var[1], var[2], var[3], var[5] = 0.0, -1.0, np.nan, var[4]         # not counted; a tie in the variance
        check_stats(eval_loc.coord_stats(r, var, n_outside=2), lr.coord_stats(r, var, n_outside=2), n)
    assert [b['n'] for b in lr.coord_stats(np.zeros(7), np.ones(7))['sigma_bins']] == [1, 1, 2, 1, 2]
    assert eval_loc.COVERAGE_LEVELS == lr.LEVELS and eval_loc.COVERAGE_Q == lr.QUANTILES
    assert eval_loc.LOC_DTYPE == lr.LOC_DTYPE and eval_loc.LOC_DTYPE.itemsize == 24


def test_quantile_literals():
    nd = statistics.NormalDist()
    assert len(lr.LEVELS) == 11 and lr.LEVELS[:9] == tuple(k / 10 for k in range(1, 10)) and lr.LEVELS[9:] == (0.95, 0.99)
    for P, q in zip(lr.LEVELS, lr.QUANTILES):
        assert abs(q - nd.inv_cdf((1 + P) / 2)) <= 1e-15, (P, q)


def test_auroc_by_hand():
    from byolo import eval_loc
    for impl in (lr.auroc_fp, eval_loc.auroc_fp):
        assert impl([1.0, 1.0], [1.0, 1.0, 1.0]) == 0.5                        # all ties
        assert impl([3.0, 4.0], [1.0, 2.0]) == 1.0 and impl([0.1], [1.0, 2.0]) == 0.0
        assert math.isnan(impl([], [1.0])) and math.isnan(impl([1.0], [])) and math.isnan(impl([np.nan], [1.0]))
        assert impl([2.0, 0.0, np.nan], [1.0, 2.0, np.inf]) == (2 + 1 + 0 + 0) / 8      # (2>1, 2=2, 0<1, 0<2) over 2 x 2 finite pairs
    rng = np.random.default_rng(1)
    a, b = rng.integers(0, 20, 150).astype(f32), rng.integers(5, 30, 90).astype(f32)
    assert eval_loc.auroc_fp(a, b) == lr.auroc_fp(a, b)


def test_inversion_recovers_a_planted_t():
    """Boxes decoded in float32 from known (t, cell, prior): the t recovered in float64 is within
    4 * 2^-23 * (l / (p (1 - p)) + 1 + |t|), twice what the roundings of the centre, of centre * l, of the corners and of one log
    add up to (for w and h: p of x and of y, l of that axis).  Priors of 0.5 .. 2 keep |corner| / size below 16."""
    rng = np.random.default_rng(5)
    worst = 0.0
    for _ in range(2000):
        lh, lw = int(rng.integers(1, 17)), int(rng.integers(1, 17))
        col, row = int(rng.integers(0, lw)), int(rng.integers(0, lh))
        p = rng.uniform(0.02, 0.98, 2)
        t = np.array([math.log(p[0] / (1 - p[0])), math.log(p[1] / (1 - p[1])), rng.uniform(-2, 2), rng.uniform(-2, 2)])
        ph, pw = f32(rng.uniform(0.5, 2.0)), f32(rng.uniform(0.5, 2.0))
        box, sx, sy = lr.decode(t.astype(f32), col, row, lh, lw, ph, pw)
        got, cell = lr.recover(box, lh, lw, ph, pw)
        assert cell == row * lw + col
        t32 = t.astype(f32).astype(f64)
        for k, (l, s) in enumerate(((lw, sx), (lh, sy), (lw, sx), (lh, sy))):
            bound = 4 * 2.0 ** -23 * (l / (s * (1 - s)) + 1 + abs(t32[k]))
            assert abs(got[k] - t32[k]) <= bound, (k, got[k], t32[k], bound)
            worst = max(worst, abs(got[k] - t32[k]) / bound)
        r, bits, c2 = lr.invert(box, box, lh, lw, ph, pw)                     # a ground truth equal to the box: no residual at all
        assert bits == 15 and c2 == cell and not r.any()
    assert worst > 0.01                                                        # the bound is not idle


def test_outside_and_degenerate_boxes():
    # the ground truth's centre in the next cell: x is counted as outside, the other three are valid
    r, bits, cell = lr.invert([0.30, 0.30, 0.40, 0.40], [0.30, 0.46, 0.40, 0.56], 4, 4, 0.1, 0.1)
    assert bits == 0b1110 and cell == 1 * 4 + 1 and r[0] == 0 and r[1] == 0 and r[3] == 0 and abs(r[2]) < 1e-6
    # zero width: the ratio is below eps
    r, bits, _ = lr.invert([0.30, 0.30, 0.40, 0.40], [0.30, 0.35, 0.40, 0.35], 4, 4, 0.1, 0.1)
    assert bits == 0b1011 and r[2] == 0
    # log ratio by hand
    r, bits, _ = lr.invert([0.25, 0.25, 0.5, 0.5], [0.25, 0.25, 0.5, 0.75], 2, 2, 0.25, 0.25)
    assert bits & 4 and r[2] == f32(math.log(2.0))


def test_generated_cases_hold_what_they_plant():
    """The seeded cases of tests/test_eval_loc_gpu.py, judged on the restatement alone."""
    seen_parity = 0
    for seed in range(12):
        ref = lr.loc_reference(seed)
        loc, table = ref['loc'], ref['table']
        tp = (loc['flags'] & 16) != 0
        ids = (loc['flags'] & 32) != 0
        assert tp.sum() >= 16 and (tp == (table['tp'] == 1)).all(), seed
        assert (tp & ~ids).sum() >= 4, seed                                    # NaN, non-integral, two out of range
        assert (tp & ids & ((loc['flags'] & 2) == 0)).sum() >= 1, seed        # a centre outside the cell (y)
        assert (tp & ids & ((loc['flags'] & 15) == 15)).sum() >= 8, seed
        red = lr.reduce_loc(table, loc, ref['variant'], ref['C'])
        assert sum(red[k][c]['n_bad_var'] for k in red if k in ('ale', 'epi') for c in lr.COORDS) >= 3, seed
        assert len(ref['batches']) == 2 and len(set(table['img'])) >= 1
        seen_parity += 1
    counts = {int(c) for s in range(12) for b in lr.loc_reference(s)['batches'] for c in b[4]}
    assert counts == {0, 1, 65, 130}
    assert any((b[1] == 96).all() for s in range(12) for b in lr.loc_reference(s)['batches'])
    assert any((b[1] == 0).any() for s in range(12) for b in lr.loc_reference(s)['batches'])
    batches, (D, obj, cls), C, variant = lr.zero_width_case()
    table, _, _ = er.match_batches(batches, obj, cls, C, unc_cols=er.UNC_COLS[variant](C), iou_thresh=0.0)
    loc = lr.loc_records(batches, table, *lr.ID_COLS[variant](C))
    assert list(table['tp']) == [1, 1] and list(table['gt']) == [0, 1]
    assert list(loc['flags'] & 15) == [0b1011, 0b1111]


# ---- the C-ABI ----------------------------------------------------------------------------------------------------------------
def test_loc_cfg_matches_the_header():
    from byolo import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "byolo.h")).read(), flags=re.S)
    body = re.search(r"typedef struct byolo_eval_loc_cfg \{(.*?)\} byolo_eval_loc_cfg;", text, flags=re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ty, names = decl.split(None, 1)
            fields += [(n.strip().split("[")[0], ty, n.count("[")) for n in names.split(",")]
    assert [n for n, _, _ in fields] == [n for n, _ in _lib.EvalLocCfg._fields_]
    L, P = _lib.EVAL_LOC_MAX_LAYERS, _lib.EVAL_LOC_MAX_PRIORS
    expect = {("int32_t", 0): ctypes.c_int32, ("int32_t", 1): ctypes.c_int32 * L, ("float", 2): (ctypes.c_float * P) * L}
    for (n, ty, dims), (_, t) in zip(fields, _lib.EvalLocCfg._fields_):
        assert t is expect[(ty, dims)], n                                       # ctypes keeps one type object per array type
    assert ctypes.sizeof(_lib.EvalLocCfg) == 4 * (4 + 3 * L + 2 * L * P)
    for macro, value in (("BYOLO_EVAL_LOC_WORDS", _lib.EVAL_LOC_WORDS), ("BYOLO_EVAL_LOC_MAX_LAYERS", L), ("BYOLO_EVAL_LOC_MAX_PRIORS", P)):
        assert re.search(r"#define\s+%s\s+%d\b" % (macro, value), text)
    assert re.search(r"#define\s+BYOLO_ABI_VERSION\s+7\b", text)
    assert _lib.lib.byolo_eval_loc_bytes(50) == 50 * 24 and _lib.lib.byolo_eval_loc_bytes(0) == 0


def test_set_loc_refuses_bad_arguments():
    from byolo import _lib, eval_loc
    lib = _lib.lib
    h = ctypes.c_void_p()
    C = 2
    cfg = _lib.EvalCfg(struct_bytes=ctypes.sizeof(_lib.EvalCfg), row_len=14 + C, obj_idx=9, cls_start_idx=11, cls_cnt=C, iou_thresh=0.5)
    buf = (ctypes.c_int32 * 64)()
    assert lib.byolo_eval_create(ctypes.byref(cfg), ctypes.cast(buf, ctypes.c_void_p), 2, ctypes.cast(buf, ctypes.c_void_p), ctypes.byref(h)) == 0
    tab = ctypes.cast(buf, ctypes.c_void_p)

    def good():
        return eval_loc.loc_cfg(12 + C, 13 + C, lr.GEOM)

    def refused(loc, needle, table=tab):
        rc = lib.byolo_eval_set_loc(h, ctypes.byref(loc), table)
        msg = lib.byolo_eval_last_error(h)
        assert rc == _lib.ERR_ARG and needle in msg, (rc, msg, needle)

    assert lib.byolo_eval_set_loc(h, ctypes.byref(good()), tab) == 0
    assert lib.byolo_eval_set_loc(h, None, None) == 0                           # off again
    c = good(); c.struct_bytes -= 4; refused(c, b"struct_bytes")
    c = good(); c.layer_col = 14 + C; refused(c, b"layer_col")
    c = good(); c.prior_col = -1; refused(c, b"prior_col")
    c = good(); c.n_layers = 0; refused(c, b"n_layers")
    c = good(); c.n_layers = 9; refused(c, b"n_layers")
    c = good(); c.n_priors[1] = 0; refused(c, b"n_priors")
    c = good(); c.n_priors[2] = 17; refused(c, b"n_priors")
    c = good(); c.lh[0] = 0; refused(c, b"grid")
    c = good(); c.lw[2] = -3; refused(c, b"grid")
    c = good(); c.prior_w[0][1] = 0.0; refused(c, b"prior")
    c = good(); c.prior_h[2][2] = float('nan'); refused(c, b"prior")
    c = good(); c.prior_h[1][0] = float('inf'); refused(c, b"prior")
    refused(good(), b"aligned", table=ctypes.c_void_p(ctypes.addressof(buf) + 2))
    assert lib.byolo_eval_set_loc(h, None, tab) == _lib.ERR_ARG and b"null cfg" in lib.byolo_eval_last_error(h)
    assert lib.byolo_eval_set_loc(None, ctypes.byref(good()), tab) == _lib.ERR_ARG
    c = good(); c.n_priors[5] = 99                                              # beyond n_layers: not looked at
    assert lib.byolo_eval_set_loc(h, ctypes.byref(c), tab) == 0
    assert lib.byolo_eval_loc_records(h, None, 0, 3, None) == _lib.ERR_ARG and b"outside the table" in lib.byolo_eval_last_error(h)
    assert lib.byolo_eval_destroy(h) == 0
    with pytest.raises(ValueError):
        eval_loc.loc_cfg(1, 2, [])
    with pytest.raises(ValueError, match='ale_x'):
        eval_loc.variance_kinds(['obj_entropy'])
    assert eval_loc.variance_kinds(['epi_x', 'epi_y', 'epi_w', 'epi_h', 'ale_x', 'ale_y', 'ale_w', 'ale_h']) == {'ale': [4, 5, 6, 7], 'epi': [0, 1, 2, 3]}
    assert eval_loc.id_columns('yolov3', 2) is None and eval_loc.id_columns('bayesian_yolov3_aleatoric', 2) == (21, 22)
