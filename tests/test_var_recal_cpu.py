"""Variance recalibration without a GPU: the numpy restatement (tests/_var_recal_ref.py) against itself, the fallback chain and
the plumbing of byolo/recalibrate.py (INTEGRATION.md "Variance recalibration")."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import _var_recal_ref as vr
from conftest import REPO

EPS = np.finfo(np.float64).eps
STEP_BOUND = 2.0 ** -25          # half a float32 ulp of the applied variance: what the consumer of v' can see


def _group(rng, n, a, b, student=False, lo=-9.0, hi=1.0):
    """n entries whose variance is miscalibrated as r^2 ~ a v^b z^2."""
    v = np.exp(rng.uniform(lo, hi, n))
    z = rng.standard_t(3, n) if student else rng.standard_normal(n)
    return np.sqrt(a * v ** b) * z, v


# ---- the restatement against itself ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("a,b", [(1.0, 1.0), (2.25, 1.0), (0.3, 0.5), (4.0, 1.75), (1.5, 0.0), (0.02, 3.0)])
def test_power_returns_a_planted_law(a, b):
    """r^2 = a v^b exactly (in float64): the gradient vanishes at (a, b) and the fit returns it."""
    rng = np.random.default_rng(11)
    v = np.exp(rng.uniform(-9.0, 1.0, 4000))
    r = np.sqrt(a * v ** b) * rng.choice([-1.0, 1.0], len(v))
    f = vr.fit_group(r, v, 'power')
    assert f['status'] == vr.FITTED and f['converged'] and f['n'] == len(v)
    err = abs(math.log(f['a']) - math.log(a)) + abs(f['b'] - b) * f['U']
    print('planted (%g, %g): |dlog a| + |db| U = %.3g after %d iterations' % (a, b, err, f['iterations']))
    assert err <= STEP_BOUND


@pytest.mark.parametrize("n", [400, 5000, 20000])
def test_scale_on_gaussian_residuals(n):
    """z ~ N(0, 1), r = s sqrt(v) z: a / s^2 is the mean of z^2, within 4 sqrt(2 / n) of 1 (the rule of tests/test_eval_loc_cpu.py);
    with the fitted a the in-sample mean of z^2 is 1."""
    rng = np.random.default_rng(100 + n)
    s2 = 2.1 ** 2
    r, v = _group(rng, n, s2, 1.0)
    f = vr.fit_group(r, v, 'scale')
    assert f['status'] == vr.FITTED and f['b'] == 1.0 and f['a'] == f['mean_z2_before']
    assert abs(f['a'] / s2 - 1.0) <= 4.0 * math.sqrt(2.0 / n)
    after = vr.fixed_sum(r * r / (f['a'] * v)) / n
    assert abs(after - 1.0) <= 64 * EPS


@pytest.mark.parametrize("seed", range(6))
def test_scale_nll_identity(seed):
    """nll_before - nll_after = 0.5 (a - 1 - log a) for the closed-form a."""
    rng = np.random.default_rng(300 + seed)
    n = int(rng.integers(3, 3000))
    r, v = _group(rng, n, float(np.exp(rng.uniform(-3, 3))), 1.0, student=bool(seed % 2))
    f = vr.fit_group(r, v, 'scale')
    a = f['a']
    got, want = f['nll_before'] - f['nll_after'], 0.5 * (a - 1.0 - math.log(a))
    assert abs(got - want) <= 64 * EPS * max(1.0, abs(f['nll_before']), abs(f['nll_after'])), (got, want)


def sweep_groups():
    """The 300 groups of the Newton sweep: n 3 .. 20000, planted b 0 .. 3, Gaussian and Student-t(3) residuals; every other group
    is also fitted in reversed table order (another summation order of the same entries)."""
    rng = np.random.default_rng(2024)
    for k in range(300):
        n = int(round(math.exp(rng.uniform(math.log(3), math.log(20000)))))
        a, b = float(np.exp(rng.uniform(-3, 3))), float(rng.uniform(0.0, 3.0))
        r, v = _group(rng, n, a, b, student=bool(k % 2))
        yield k, (r[::-1], v[::-1]) if k % 4 >= 2 else (r, v)


def test_newton_sweep_ends_at_the_stationary_point():
    """The Newton step AT every answer, its sums taken exactly (math.fsum), is at most 2^-25 long: half a float32 ulp of the applied
    variance.  (Measured: worst 3.84e-15, at most 23 iterations; profiles/var_recal.md.)"""
    worst, most_iter, fitted = 0.0, 0, 0
    for k, (r, v) in sweep_groups():
        f = vr.fit_group(r, v, 'power')
        assert f['status'] == vr.FITTED and f['converged'] and f['iterations'] <= 100, (k, f)
        fitted += 1
        size = vr.exact_step_size(r, v, f['a'], f['b'])
        worst, most_iter = max(worst, size), max(most_iter, f['iterations'])
        assert size <= STEP_BOUND, (k, size, f)
    print('newton sweep: %d of 300 fitted, worst exact step %.3g, at most %d iterations' % (fitted, worst, most_iter))
    assert fitted == 300


def test_degenerate_groups():
    rng = np.random.default_rng(5)
    r, v = _group(rng, 500, 2.0, 1.0)
    same = vr.fit_group(r, np.full(500, 0.25), 'power')            # one variance for all: b cannot be told, the Hessian is singular
    assert same['status'] == vr.SCALE_FALLBACK and same['b'] == 1.0 and same['converged']
    assert same['a'] == vr.fit_group(r, np.full(500, 0.25), 'scale')['a']
    for method in ('scale', 'power'):
        zero = vr.fit_group(np.zeros(500), v, method)                # all-zero residuals: the identity, not a = 0
        assert zero['status'] == vr.IDENTITY and (zero['a'], zero['b']) == (1.0, 1.0)
        assert zero['nll_after'] == zero['nll_before']
        two = vr.fit_group(r[:2], v[:2], method)
        assert two['status'] == (vr.FITTED if method == 'scale' else vr.SCALE_FALLBACK) and two['b'] == 1.0
        none = vr.fit_group(r[:0], v[:0], method)
        assert none['status'] == vr.EMPTY and none['n'] == 0
    inf = vr.fit_group(np.array([1e200, 1.0, 1.0]), np.array([1e-200, 1.0, 1.0]), 'scale')          # sum r^2 / v overflows
    assert inf['status'] == vr.IDENTITY and inf['a'] == 1.0


def test_fixed_sum_is_the_stated_order():
    rng = np.random.default_rng(1)
    for n in (0, 1, 255, 256, 257, 1000):
        x = rng.standard_normal(n) * np.exp(rng.uniform(-20, 20, n))
        partial = [0.0] * 256
        for j in range(n):
            partial[j % 256] += float(x[j])
        total = 0.0
        for t in range(256):
            total += partial[t]
        assert vr.fixed_sum(x) == total, n


def test_closed_loop_on_the_seeded_loc_cases():
    """measure -> fit(by='all', 'scale') -> apply -> measure on the 12 cases of tests/_eval_loc_ref.py, all in numpy: every case keeps
    its n and reads mean z^2 = 1 within 2^-23, one float32 rounding of each variance (tests/test_var_recal_gpu.py relies on it)."""
    import _eval_loc_ref as lr
    worst = 0.0
    for seed in range(12):
        ref = lr.loc_reference(seed)
        for target in (('ale',) if ref['variant'] == 'yolov3_aleatoric' else ('ale', 'epi', 'total')):
            for n0, n1, a, mz2 in vr.loc_closed_loop(ref, target)[0]:
                assert n0 == n1 > 0 and abs(mz2 - 1.0) <= 2.0 ** -23, (seed, target, n0, n1, a, mz2)
                worst = max(worst, abs(mz2 - 1.0))
    print('closed loop on the CPU: worst |mean_z2 - 1| = %.3g' % worst)


# ---- the fallback chain ----------------------------------------------------------------------------------------------------------
def _segments(groups, method):
    """fit_arrays' result from the restatement: groups {group number: {coordinate: (r, v)}}."""
    from byolo import recalibrate as rc
    names = ('n', 'a', 'b', 'mean_z2_before', 'nll_before', 'nll_after', 'iterations', 'status', 'converged')
    seg = {k: [None] * (rc.N_GROUPS * 4) for k in names}
    empty = np.zeros(0)
    for g in range(rc.N_GROUPS):
        for c in range(4):
            f = vr.fit_group(*groups.get(g, {}).get(c, (empty, empty)), method)
            for k in names:
                seg[k][g * 4 + c] = f[k]
    return {k: np.array(v) for k, v in seg.items()}


@pytest.mark.parametrize("method", ["scale", "power"])
def test_fallback_chain(method):
    """prior -> layer -> all -> identity by min_n, per coordinate."""
    from byolo import recalibrate as rc
    rng = np.random.default_rng(77)
    n_priors = [3, 3]
    big, small = _group(rng, 150, 3.0, 1.0), _group(rng, 20, 0.5, 1.0)
    tiny = _group(rng, 5, 9.0, 1.0)
    cat = lambda *gs: (np.concatenate([g[0] for g in gs]), np.concatenate([g[1] for g in gs]))
    groups = {rc._g_prior(0, 0): {0: big, 1: small, 2: small, 3: tiny},
              rc._g_prior(0, 1): {0: small, 1: small, 2: small},
              rc._g_layer(0): {0: cat(big, small), 1: cat(small, small), 2: cat(small, small), 3: tiny},      # (coordinate 1: 40 < 100)
              rc._g_layer(1): {},
              rc.G_ALL: {0: cat(big, small), 1: cat(small, small, big), 2: cat(small, small), 3: tiny}}
    # coordinate 2: nobody reaches min_n; coordinate 3 neither
    seg = _segments(groups, method)
    cal = rc.resolve(seg, 'yolov3_aleatoric', n_priors, 'ale', 'prior', method, 100)
    rep = {(e['layer'], e['prior'], e['coord']): e for e in cal.report}
    assert len(cal.report) == 6 * 4
    assert rep[(0, 0, 'x')]['source'] == 'prior' and rep[(0, 0, 'x')]['n'] == 150
    assert cal.a[0][0][0] == seg['a'][rc._g_prior(0, 0) * 4] and cal.b[0][0][0] == seg['b'][rc._g_prior(0, 0) * 4]
    assert rep[(0, 1, 'x')]['source'] == 'layer' and rep[(0, 1, 'x')]['n'] == 20
    assert cal.a[0][1][0] == seg['a'][rc._g_layer(0) * 4]
    assert rep[(0, 0, 'y')]['source'] == 'all' and cal.a[0][0][1] == seg['a'][rc.G_ALL * 4 + 1]
    assert rep[(1, 2, 'x')]['source'] == 'all' and rep[(1, 2, 'x')]['n'] == 0 and cal.a[1][2][0] == seg['a'][rc.G_ALL * 4]
    for c, name in ((2, 'w'), (3, 'h')):
        for l in range(2):
            for p in range(3):
                assert rep[(l, p, name)]['source'] == 'identity' and (cal.a[l][p][c], cal.b[l][p][c]) == (1.0, 1.0)
    # the coarser groupings: one line per layer / one for everything, every prior of the group gets its pair
    by_layer = rc.resolve(seg, 'yolov3_aleatoric', n_priors, 'ale', 'layer', method, 100)
    assert len(by_layer.report) == 2 * 4 and [by_layer.a[0][p][0] for p in range(3)] == [float(seg['a'][rc._g_layer(0) * 4])] * 3
    assert by_layer.report[0]['prior'] is None and by_layer.a[1][0][0] == seg['a'][rc.G_ALL * 4]
    by_all = rc.resolve(seg, 'yolov3_aleatoric', n_priors, 'ale', 'all', method, 100)
    assert len(by_all.report) == 4 and by_all.report[0]['layer'] is None and by_all.a[1][2][1] == seg['a'][rc.G_ALL * 4 + 1]
    # min_n = 1: every group with an entry stands for itself
    own = rc.resolve(seg, 'yolov3_aleatoric', n_priors, 'ale', 'prior', method, 1)
    assert {e['source'] for e in own.report if e['n'] > 0} == {'prior'}


def test_degenerate_groups_through_the_chain():
    from byolo import recalibrate as rc
    rng = np.random.default_rng(78)
    r, v = _group(rng, 200, 2.0, 1.0)
    groups = {rc.G_ALL: {0: (r, np.full(200, 0.5)), 1: (np.zeros(200), v), 2: (r, v)}}
    cal = rc.resolve(_segments(groups, 'power'), 'bayesian_yolov3_aleatoric', [3, 3, 3], 'total', 'all', 'power', 100)
    x, y, w, h = cal.report
    assert (x['source'], x['status'], x['b']) == ('all', 'scale_fallback', 1.0) and x['a'] > 0
    assert (y['source'], y['status'], y['a'], y['b']) == ('all', 'identity', 1.0, 1.0)
    assert (w['source'], w['status'], w['converged']) == ('all', 'fit', True) and w['iterations'] >= 1
    assert (h['source'], h['n']) == ('identity', 0)


# ---- plumbing --------------------------------------------------------------------------------------------------------------------
def _random_cal(rng, variant='bayesian_yolov3_aleatoric', n_priors=(3, 3, 3), **kw):
    from byolo.recalibrate import VarCalibration
    a = [[[float(x) for x in np.exp(rng.uniform(-30, 30, 4))] for _ in range(p)] for p in n_priors]
    b = [[[float(x) for x in rng.uniform(-2, 4, 4)] for _ in range(p)] for p in n_priors]
    return VarCalibration(variant, list(n_priors), a=a, b=b, **kw)


def test_json_round_trip_is_bit_exact(tmp_path):
    from byolo.recalibrate import VarCalibration
    rng = np.random.default_rng(9)
    cal = _random_cal(rng, target='epi', by='layer', method='power', min_n=7,
                      report=[{'layer': 0, 'prior': None, 'coord': 'x', 'n': 3, 'source': 'all', 'status': 'fit', 'a': 0.1 + 0.2, 'b': 1e-300,
                               'mean_z2_before': math.nan, 'nll_before': 5e-324, 'nll_after': -1.0 / 3.0, 'iterations': 3, 'converged': True}])
    cal.a[0][0][0], cal.b[2][2][3] = 5e-324, float(np.nextafter(1.0, 2.0))
    bits = lambda t: [np.float64(v).view(np.uint64) for l in t for p in l for v in p]
    for back in (VarCalibration.from_json(cal.to_json()), None):
        if back is None:
            cal.save(str(tmp_path / 'var_recal.json'))
            back = VarCalibration.load(str(tmp_path / 'var_recal.json'))
        assert bits(back.a) == bits(cal.a) and bits(back.b) == bits(cal.b)
        assert (back.variant, back.n_priors, back.target, back.by, back.method, back.min_n) == ('bayesian_yolov3_aleatoric', [3, 3, 3], 'epi', 'layer', 'power', 7)
        e, o = back.report[0], cal.report[0]
        assert e['mean_z2_before'] is None and all(e[k] == o[k] for k in o if k != 'mean_z2_before')
        assert back.to_json() == cal.to_json()
    assert VarCalibration.coerce(cal) is cal and VarCalibration.coerce(str(tmp_path / 'var_recal.json')).a == cal.a
    import json
    assert VarCalibration.coerce(json.loads(cal.to_json())).b == cal.b


def test_ctypes_struct_matches_the_header():
    from byolo import _lib
    from test_abi import _header_functions
    hdr = _header_functions()
    new = {"byolo_var_recal_table": 2, "byolo_var_recal_apply": 7, "byolo_set_var_recal": 2, "byolo_var_recal_fit_workspace_bytes": 1, "byolo_var_recal_fit": 10}
    for name, arity in new.items():
        assert name in hdr and name in _lib.PROTOTYPES, name
        assert len(hdr[name][1]) == len(_lib.PROTOTYPES[name][1]) == arity, name
        assert getattr(_lib.lib, name)
    text = open(os.path.join(REPO, "include", "byolo.h")).read()
    assert re.search(r"#define BYOLO_ABI_VERSION 7\b", text) and _lib.lib.byolo_abi_version() == 7 == _lib.ABI_VERSION
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct byolo_var_recal_cfg \{(.*?)\} byolo_var_recal_cfg;", text, flags=re.S).group(1), flags=re.S)
    dims = {"BYOLO_EVAL_LOC_MAX_LAYERS": _lib.EVAL_LOC_MAX_LAYERS, "BYOLO_EVAL_LOC_MAX_PRIORS": _lib.EVAL_LOC_MAX_PRIORS, "4": 4}
    fields = []
    for decl in body.split(";"):
        if not decl.strip():
            continue
        ty, names = decl.strip().split(None, 1)
        for n in names.split(","):
            name, *shape = re.split(r"[\[\]]+", n.strip().rstrip("]"))
            t = {"int32_t": ctypes.c_int32, "double": ctypes.c_double}[ty]
            for d in reversed(shape):
                t = t * dims[d]
            fields.append((name, t))
    assert [n for n, _ in fields] == [n for n, _ in _lib.VarRecalCfg._fields_] and fields[0][0] == "struct_bytes"
    for (n, t), (_, u) in zip(fields, _lib.VarRecalCfg._fields_):
        assert ctypes.sizeof(t) == ctypes.sizeof(u) and getattr(t, '_length_', None) == getattr(u, '_length_', None), n
    for name, value in (("BYOLO_VAR_RECAL_TABLE_BYTES", _lib.VAR_RECAL_TABLE_BYTES), ("BYOLO_VAR_RECAL_FIT_WORDS", _lib.VAR_RECAL_FIT_WORDS)):
        assert re.search(r"#define %s %d\b" % (name, value), text), name
    assert re.search(r"enum \{ BYOLO_VAR_RECAL_ALE = 1, BYOLO_VAR_RECAL_EPI = 2, BYOLO_VAR_RECAL_TOTAL = 3 \}", text)
    assert re.search(r"enum \{ BYOLO_VAR_RECAL_SCALE = 0, BYOLO_VAR_RECAL_POWER = 1 \}", text)
    assert re.search(r"enum \{ BYOLO_VAR_RECAL_FITTED = 0, BYOLO_VAR_RECAL_SCALE_FALLBACK = 1, BYOLO_VAR_RECAL_IDENTITY = 2, BYOLO_VAR_RECAL_EMPTY = 3 \}", text)
    assert (_lib.VAR_RECAL_ALE, _lib.VAR_RECAL_EPI, _lib.VAR_RECAL_TOTAL, _lib.VAR_RECAL_SCALE, _lib.VAR_RECAL_POWER) == (1, 2, 3, 0, 1)
    assert (vr.FITTED, vr.SCALE_FALLBACK, vr.IDENTITY, vr.EMPTY) == (_lib.VAR_RECAL_FITTED, _lib.VAR_RECAL_SCALE_FALLBACK, _lib.VAR_RECAL_IDENTITY, _lib.VAR_RECAL_EMPTY)
    # the table of a VarCalibration lands where the header says
    cal = _random_cal(np.random.default_rng(3), n_priors=(2, 16))
    cfg = cal.cfg()
    assert cfg.struct_bytes == ctypes.sizeof(_lib.VarRecalCfg) == 16 + 32 + 2 * 8 * 16 * 4 * 8
    assert (cfg.kind, cfg.target, cfg.n_layers, list(cfg.n_priors)[:3]) == (_lib.DET_EPISTEMIC, _lib.VAR_RECAL_TOTAL, 2, [2, 16, 0])
    assert cfg.a[1][15][3] == cal.a[1][15][3] and cfg.b[0][1][2] == cal.b[0][1][2]


def test_invalid_settings_name_the_field():
    from byolo.recalibrate import VarCalibration
    ok = dict(variant='bayesian_yolov3_aleatoric', n_priors=[3, 3, 3])
    ident = [[[1.0] * 4] * 3] * 3
    for kw, field in ((dict(variant='yolov3'), 'variant'), (dict(target='sum'), 'target'), (dict(by='class'), 'by'),
                      (dict(method='isotonic'), 'method'), (dict(min_n=0), 'min_n'), (dict(min_n=2.5), 'min_n'),
                      (dict(n_priors=[]), 'n_layers'), (dict(n_priors=[3] * 9), 'n_layers'), (dict(n_priors=[3, 17]), 'n_priors'),
                      (dict(variant='yolov3_aleatoric', target='total'), 'target'), (dict(variant='yolov3_aleatoric', target='epi'), 'target'),
                      (dict(a=[[[1.0] * 4] * 3] * 2), 'a has'), (dict(b=[[[1.0] * 3] * 3] * 3), 'b[0][0]'),
                      (dict(a=[[[1.0, 0.0, 1.0, 1.0]] * 3] * 3), 'a[0][0][1]'), (dict(a=[[[1.0, 1.0, -2.0, 1.0]] * 3] * 3), 'a[0][0][2]'),
                      (dict(a=[[[math.inf] * 4] * 3] * 3), 'a[0][0][0]'), (dict(b=[[[1.0, 1.0, 1.0, math.nan]] * 3] * 3), 'b[0][0][3]')):
        with pytest.raises(ValueError, match=re.escape(field)):
            VarCalibration(**dict(dict(ok, a=ident, b=ident), **kw))
    import evaluate
    import recalibrate
    from lib_yolo import yolov3
    base = {'full_img_size': [64, 96, 3], 'cls_cnt': 2, 'batch_size': 3, 'crop': False, 'priors': yolov3.ECP_9_PRIORS, 'T': 3, 'weights': 'synthetic',
            'implicit_background_class': True, 'data': {'file_pattern': 'x-*'}, 'out_path': 'no'}
    assert evaluate.check_config(dict(base, var_recal='c.json'), 'bayesian')['engine_options'] == {'var_recal': 'c.json'}
    assert 'engine_options' not in evaluate.check_config(dict(base, var_recal='c.json', var_recal_compare=True), 'bayesian')
    assert 'var_recal' not in evaluate.check_config(base, 'bayesian')
    for kw in (dict(var_recal_compare=True), dict(var_recal='c.json', var_recal_compare=True, box_vote=True, box_vote_compare=True),
               dict(var_recal='c.json', var_recal_compare=True, soft_nms_compare=True), dict(var_recal='c.json', var_recal_compare=True, box_vote=True),
               dict(var_recal=3), dict(var_recal='c.json', var_recal_compare='yes')):
        with pytest.raises(ValueError, match='var_recal'):
            evaluate.check_config(dict(base, **kw), 'bayesian')
    with pytest.raises(ValueError, match='var_recal'):
        evaluate.check_config(dict(base, var_recal='c.json'), 'standard')
    ok_cfg = recalibrate.check_config(base, 'aleatoric')
    assert (ok_cfg['recal_by'], ok_cfg['recal_method'], ok_cfg['recal_min_n'], ok_cfg['recal_holdout'], ok_cfg['localisation']) == ('prior', 'scale', 100, None, True)
    for kw, field in ((dict(recal_holdout=1), 'recal_holdout'), (dict(recal_method='isotonic'), 'recal_method'), (dict(recal_by='class'), 'recal_by'),
                      (dict(recal_min_n=0), 'recal_min_n'), (dict(recal_target='sum'), 'recal_target'), (dict(recal_target='total'), 'recal_target'),
                      (dict(var_recal='c.json'), 'var_recal'), (dict(box_vote=True), 'box_vote'), (dict(localisation=False), 'localisation')):
        with pytest.raises(ValueError, match=field):
            recalibrate.check_config(dict(base, **kw), 'aleatoric')
    with pytest.raises(ValueError, match='standard'):
        recalibrate.check_config(base, 'standard')
    with pytest.raises(ValueError, match='format'):
        VarCalibration.from_json('{"a": 1}')
    with pytest.raises(ValueError, match="'method'"):
        VarCalibration.from_json('{"format": "byolo_var_recal", "variant": "yolov3_aleatoric", "n_priors": [3], "target": "ale", "by": "all", "a": [], "b": []}')
    with pytest.raises(ValueError):
        VarCalibration.coerce(3)
    assert VarCalibration('yolov3_aleatoric', [3]).target == 'ale' and VarCalibration(**ok).target == 'total'
    assert VarCalibration(**ok).is_identity and not _random_cal(np.random.default_rng(0)).is_identity


def test_a_calibration_of_another_model_is_refused(tmp_path):
    """Variant and geometry are checked when a calibration is loaded into a model, by name; the library checks again."""
    from byolo import _lib
    from byolo.recalibrate import VarCalibration
    from conftest import build_model
    rng = np.random.default_rng(4)
    path = str(tmp_path / 'cal.json')
    _random_cal(rng).save(path)
    _, m = build_model('bayesian_yolov3_aleatoric', 64, 96, engine_options={'var_recal': path})      # the option of the model classes
    eng = m.engine
    assert eng._var_recal.a == VarCalibration.load(path).a
    eng.set_var_recal(None)
    assert eng._var_recal is None
    for cal, field in ((_random_cal(rng, 'yolov3_aleatoric', target='ale'), 'variant'), (_random_cal(rng, n_priors=(3, 3)), 'n_layers'),
                       (_random_cal(rng, n_priors=(3, 3, 4)), 'n_priors')):
        with pytest.raises(ValueError, match=field):
            eng.set_var_recal(cal)
        with pytest.raises(ValueError, match=field):
            build_model('bayesian_yolov3_aleatoric', 64, 96, engine_options={'var_recal': cal})
    assert eng._var_recal is None
    # the C-ABI itself: the struct's size, the kind and the geometry of the handle
    cfg = _random_cal(rng).cfg()
    check = lambda c: (_lib.lib.byolo_set_var_recal(eng._h, ctypes.byref(c)), (_lib.lib.byolo_last_error(eng._h) or b'').decode())
    assert check(cfg)[0] == 0
    cfg.struct_bytes -= 8
    rc, msg = check(cfg)
    assert rc == _lib.ERR_ARG and 'struct_bytes' in msg
    cfg.struct_bytes += 8
    for field, value, word in (('kind', _lib.DET_ALEATORIC, 'target'), ('kind', 0, 'kind'), ('target', 4, 'target'), ('n_layers', 2, 'n_layers'), ('n_layers', 9, 'n_layers')):
        keep = getattr(cfg, field)
        setattr(cfg, field, value)
        rc, msg = check(cfg)
        assert rc == _lib.ERR_ARG and word in msg, (field, value, msg)
        setattr(cfg, field, keep)
    cfg.n_priors[1] = 4
    for k in range(4):
        cfg.a[1][3][k] = cfg.b[1][3][k] = 1.0
    rc, msg = check(cfg)
    assert rc == _lib.ERR_ARG and 'n_priors' in msg
    cfg.n_priors[1] = 3
    cfg.a[2][2][3] = 0.0
    rc, msg = check(cfg)
    assert rc == _lib.ERR_ARG and 'a[2][2][3]' in msg
    cfg.a[2][2][3] = 1.0
    cfg.b[0][1][0] = math.inf
    rc, msg = check(cfg)
    assert rc == _lib.ERR_ARG and 'b[0][1][0]' in msg
    assert _lib.lib.byolo_set_var_recal(eng._h, None) == 0
    _, ale = build_model('yolov3_aleatoric', 64, 96)
    rc = _lib.lib.byolo_set_var_recal(ale.engine._h, ctypes.byref(_random_cal(rng).cfg()))
    assert rc == _lib.ERR_ARG and b'kind' in _lib.lib.byolo_last_error(ale.engine._h)
    _, std = build_model('yolov3', 64, 96)
    with pytest.raises(ValueError, match='variant'):
        std.engine.set_var_recal(_random_cal(rng))
    for e in (eng, ale.engine, std.engine):
        e.close()
