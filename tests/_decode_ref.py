"""Inputs, float64 reference and mutations for the decode / MC-reduction stage (csrc/tail_kernels.hip: decode_std_kernel,
decode_ale_kernel, decode_epi_kernel, epi_stats_kernel).  No GPU in here: tests/test_decode_f64_cpu.py proves the inputs and the
assertion on the CPU, tests/test_decode_f64_gpu.py puts the device's rows through the same assertion.

REFERENCE   oracle/cpu_ref.py's decode_* follow the dtype of the logits: the float32 logits cast to float64 give the reference,
            the same logits in float32 give the floor F(g); the contract is oracle/report.py's, as it stands (device vs float64 at
            allowance(floor), vs float32 at allowance(floor, "float32"), ids exact, NaN / inf patterns equal).  No constant of
            this module's own bounds the device.
INPUTS      chosen so that NOTHING has to be left out of the comparison (tools/soak_decode.py needs three exclusion bands):
            spread  clip(2 N(0,1), -12, 12): no logit near the bands where float32 and float64 disagree about saturation
            agree   one draw per image + 1e-3 N(0,1) per sample, the MC-dropout regime: mutual information and epistemic
                    variance are small differences of large terms
            plants  four lanes, written into EVERY sample of the lane so that the mean saturates too: all +800, all -800,
                    +-800 alternating along the channels, and one sample's four location logits at 30 (one-pass cancellation
                    without overflow).  At +-800 float32 and float64 agree: exp overflows / underflows in both, the sigmoid is
                    exactly 0 or 1 in both (at +-120 float64 keeps exp(-120) and the NaN patterns differ).
            Non-square grids, three distinct priors with ph != pw (dyadic: the device's float32 copies are exact), layer ids
            0 .. 2, the layer's block in the middle of a buffer filled with a sentinel.
MUTATIONS   `restate` is the stage once more in plain float64 numpy with one switch per wrong kernel (MUTATIONS)."""
import collections
import functools

import numpy as np

from oracle import cpu_ref
from oracle.report import RTOL, rows_report, allowance

VARIANTS = cpu_ref.VARIANTS
PRIORS = [(0.3125, 0.109375), (0.15625, 0.21875), (0.0625, 0.046875)]        # (ph, pw), exact in float32
SENTINEL = np.float32(-777.25)
EXACT_C = (1, 2, 3, 4, 8, 80)                     # launch_decode: builds whose class count is a compile-time constant
CAPACITY_C = (5, 9, 24, 25, 48, 49, 81, 128)      # capacity builds of 8 / 24 / 48 / 128 slots: both sides of every boundary

Case = collections.namedtuple("Case", "kind C B T lh lw regime layer_id box_base tail seed")


def case_id(c):
    return "kind%d-C%d-%s-B%d-T%d-%dx%d" % (c.kind, c.C, c.regime, c.B, c.T, c.lh, c.lw)


def make_case(kind, C, regime="spread", T=None, B=2, lh=5, lw=7, seed=0):
    if T is None:
        T = 1 if kind < 2 else (7 if regime == "spread" else 50)
    return Case(kind, C, B, T, lh, lw, regime, (kind + C) % 3, 3 + C % 5, 2 + C % 3, seed)


def build_cases():
    """Every build of the three decode kernels (the GPU test's first block): kinds 0 .. 2 x the exact and the capacity class
    counts, B = 2, grid 5 x 7; spread (T = 7 for kind 2), and for kind 2 also agree (T = 50) and a single pass (T = 1)."""
    out = []
    for kind in (0, 1, 2):
        for C in EXACT_C + CAPACITY_C:
            out.append(make_case(kind, C))
            if kind == 2:
                out.append(make_case(kind, C, "agree"))
                out.append(make_case(kind, C, "spread", T=1))
    return out


# launch_decode_c caps the grid at 4096 x 256 = 1 048 576 lanes: B = 2 images of 421 x 419 x 3 are 1 058 394, so the last 9 818
# lanes (image 1, the final cells -- the -800 plant among them) are the second trip of the grid-stride loop
STRIDE_LANES = 4096 * 256
STRIDE_GRID = dict(B=2, lh=421, lw=419)


def stride_cases():
    return [make_case(0, 1, **STRIDE_GRID), make_case(1, 2, **STRIDE_GRID), make_case(2, 2, T=2, **STRIDE_GRID)]


def geometry(c):
    """(F, blk, D): channels of the raw tensor, channels per prior, columns of a row."""
    blk = (5 + c.C) * (1 if c.kind == 0 else 2)
    return 3 * blk, blk, cpu_ref.row_layout(VARIANTS[c.kind], c.C)[0]


def n_rows(c):
    return 3 * c.lh * c.lw


def n_total(c):
    return c.box_base + n_rows(c) + c.tail


def plant_lanes(c):
    """(image, row, col, prior, what) of the four planted lanes."""
    lanes = [(0, 0, 0, 0, "+800"), (0, c.lh // 2, c.lw // 2, 1, "alt"), (c.B - 1, min(1, c.lh - 1), c.lw - 2, 0, "30"),
             (c.B - 1, c.lh - 1, c.lw - 1, 2, "-800")]
    assert len({l[:4] for l in lanes}) == 4, "the grid is too small for four distinct plants"
    return lanes


def make_raw(c):
    """float32 logits [B * T, lh, lw, F], sample s = image * T + t."""
    F, blk, _ = geometry(c)
    g = np.random.default_rng([c.seed, c.kind, c.C, c.T, c.lh, c.lw, c.B, len(c.regime)])
    shape = (c.B, c.T, c.lh, c.lw, F)
    if c.regime == "spread":
        raw = np.clip(2.0 * g.standard_normal(shape, dtype=np.float32), -12.0, 12.0)
    else:
        base = np.clip(2.0 * g.standard_normal((c.B, 1, c.lh, c.lw, F), dtype=np.float32), -12.0, 12.0)
        raw = base + np.float32(1e-3) * g.standard_normal(shape, dtype=np.float32)
    raw = np.ascontiguousarray(raw, dtype=np.float32)
    r6 = raw.reshape(c.B, c.T, c.lh, c.lw, 3, blk)
    alt = np.where(np.arange(blk) % 2 == 0, 800.0, -800.0).astype(np.float32)
    for b, row, col, pr, what in plant_lanes(c):
        if what == "+800":
            r6[b, :, row, col, pr, :] = 800.0
        elif what == "-800":
            r6[b, :, row, col, pr, :] = -800.0
        elif what == "alt":
            r6[b, :, row, col, pr, :] = alt
        else:
            r6[b, c.T // 2, row, col, pr, 0:4] = 30.0
    return raw.reshape(c.B * c.T, c.lh, c.lw, F)


def band_count(c, raw):
    """Elements a comparison against float32 would have to leave out -- the three bands of tools/soak_decode.py: objectness with
    |x| in 15.5 .. 18.5 (float32's sigmoid rounds to 1 there, float64's does not) or 85 .. 106 (exp underflows in float32 alone);
    a class logit that far below its row's maximum; a log-variance whose exp is a float32 denormal or underflows in float32 alone
    (-745 < x < -87).  The inputs above have none; kind 0 has no entropy and no exp(logvar), so no band."""
    if c.kind == 0:
        return 0
    _, blk, _ = geometry(c)
    r6 = raw.reshape(c.B, c.T, c.lh, c.lw, 3, blk).astype(np.float64)
    xo = np.abs(r6[..., 8])
    n = int((((xo > 15.5) & (xo < 18.5)) | ((xo > 85.0) & (xo < 106.0))).sum())
    cl = r6[..., 10:10 + c.C]
    dd = cl.max(-1, keepdims=True) - cl
    n += int(((dd > 85.0) & (dd < 106.0)).sum())
    lv = r6[..., 4:8]
    n += int(((lv < -87.0) & (lv > -745.0)).sum())
    return n


def oracle_rows(c, raw, dtype):
    """The layer's rows [B, 3 * lh * lw, D] from oracle/cpu_ref.py in `dtype` (prior-major, concat_bbox's order)."""
    import torch
    rt = torch.from_numpy(raw).to(dtype)
    with torch.no_grad():
        if c.kind == 0:
            rows = cpu_ref.concat_bbox([cpu_ref.decode_standard(rt, PRIORS, c.C)], True)
        elif c.kind == 1:
            rows = cpu_ref.concat_bbox([cpu_ref.decode_aleatoric(rt, PRIORS, c.C, c.layer_id)], True)
        else:
            rows = torch.stack([cpu_ref.concat_bbox([cpu_ref.decode_epistemic(rt[b * c.T:(b + 1) * c.T], PRIORS, c.C, c.layer_id)], False)
                                for b in range(c.B)])
    return rows.numpy()


# ---------------------------------------------------------------------------------------------
# the determinant column
# ---------------------------------------------------------------------------------------------
def det_scaled_error(got, ref, raw, B, T):
    """|got - ref| of column 12 (the determinant of the epistemic covariance) at the scale of Hadamard's bound -- the product of
    the diagonal -- of the matrix float32 ACTUALLY holds: every entry of the one-pass covariance E[l l^T] - E[l] E[l]^T
    (layers.py:383) carries an absolute error of a few ulps of E[l^2], so a variance of 1e-4 beside E[l^2] = 900 (three samples of a
    logit near 30) is half noise, and the determinant of the rank <= T - 1 matrix moves by that noise times a cofactor
    (tools/soak_decode.py, seed 62, case 239: T = 3, logit scale 30 -- one failure in 2 400 cases of six seeds under the bound on
    the exact diagonal, where the float32 CPU oracle happened to sit at 7e-8).  `got`, `ref` [B, 3 * lh * lw, D] prior-major, `raw`
    the float32 logits [B * T, lh, lw, F]; NaN where either side is."""
    lh, lw = raw.shape[1], raw.shape[2]
    with np.errstate(all="ignore"):
        raw5d = raw.reshape(B, T, lh, lw, 3, -1)[..., :4].astype(np.float64)
        m2d = (raw5d ** 2).mean(1).transpose(0, 3, 1, 2, 4).reshape(B, -1, 4)        # E[l^2], prior-major like concat_bbox
        hb = np.maximum(1.0, np.abs(np.prod(np.abs(ref[..., 4:8].astype(np.float64)) + 16 * 6e-8 * m2d, axis=-1)))
        return np.abs(got[..., 12].astype(np.float64) - ref[..., 12]) / hb


def _det_report(derr):
    d = np.nan_to_num(derr, nan=0.0)
    return {"det(epi covar) / Hadamard": dict(worst_in_bounds=float(d.max() / RTOL), max_abs_err=float(d.max()), max_ref=1.0)}


# ---------------------------------------------------------------------------------------------
# reference of a case, computed once
# ---------------------------------------------------------------------------------------------
def _reference(c):
    import torch
    raw = make_raw(c)
    r64 = oracle_rows(c, raw, torch.float64)
    r32 = oracle_rows(c, raw, torch.float32)
    ref = dict(raw=raw, r64=r64, r32=r32, det_floor=None)
    z64, z32 = r64, r32
    if c.kind == 2:
        ref["det_floor"] = det_scaled_error(r32, r64, raw, c.B, c.T)
        z64, z32 = r64.copy(), r32.copy()
        z64[..., 12] = 0
        z32[..., 12] = 0
    ref["z64"], ref["z32"] = z64, z32
    ref["floor"] = rows_report(z32, z64, VARIANTS[c.kind], c.C)
    for a in ref.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return ref


reference = functools.lru_cache(maxsize=None)(_reference)       # small cases: shared by every test that needs them, read-only


def buffer_with(c, rows):
    """The device's view of `rows` [B, 3 * lh * lw, D]: float32, at box_base in a buffer of sentinels."""
    buf = np.full((c.B, n_total(c), geometry(c)[2]), SENTINEL, dtype=np.float32)
    with np.errstate(over="ignore"):
        buf[:, c.box_base:c.box_base + n_rows(c)] = rows.astype(np.float32)
    return buf


def check_rows(c, buf, ref, what):
    """THE assertion: `buf` [B, n_total, D] float32 -- the buffer the device wrote, or a stand-in for it -- against the float64 and
    the float32 reference of case `c` under oracle/report.py's contract; the rows in front of and behind the layer's block still
    hold the sentinel.  Returns {"f64": report, "f32": report, "det": scaled det errors or None}."""
    from conftest import assert_rows_close, record_parity
    v = VARIANTS[c.kind]
    buf = np.asarray(buf)
    assert buf.dtype == np.float32 and buf.shape == (c.B, n_total(c), geometry(c)[2]), "%s: buffer %s %s" % (what, buf.dtype, buf.shape)
    lo, hi = c.box_base, c.box_base + n_rows(c)
    sent = SENTINEL.view(np.uint32)
    assert (buf[:, :lo].view(np.uint32) == sent).all(), "%s: rows in front of the layer's block were written" % what
    assert (buf[:, hi:].view(np.uint32) == sent).all(), "%s: rows behind the layer's block were written" % what
    got = buf[:, lo:hi]
    det = None
    if c.kind == 2:
        # the determinant as the soak handles it: NaN pattern equal, compared at Hadamard's scale, then out of the group report
        for name, r in (("float64", ref["r64"]), ("float32", ref["r32"])):
            assert np.array_equal(np.isnan(got[..., 12]), np.isnan(r[..., 12])), "%s: det NaN pattern vs %s" % (what, name)
            derr = det_scaled_error(got, r, ref["raw"], c.B, c.T)
            record_parity("%s vs the %s oracle: determinant" % (what, name), _det_report(derr))
            assert not (np.nan_to_num(derr, nan=0.0) >= RTOL).any(), "%s: det(epi covar) vs %s: scaled error %.3e" % (what, name, np.nanmax(derr))
            det = derr if det is None else det
        got = got.copy()
        got[..., 12] = 0
    for name, r in (("float64", ref["z64"]), ("float32", ref["z32"])):      # assert_rows_close's own condition, with the place
        bad = (np.isnan(got) != np.isnan(r)) | (np.isinf(got) != np.isinf(r))
        if bad.any():
            b, n, col = [int(i) for i in np.argwhere(bad)[0]]
            pr, cell = divmod(n, c.lh * c.lw)
            lane = ref["raw"].reshape(c.B, c.T, c.lh, c.lw, 3, -1)[b, :, cell // c.lw, cell % c.lw, pr]
            raise AssertionError("%s: NaN / inf pattern vs the %s oracle differs in %d elements; first: image %d, prior %d, cell (%d, %d), column %d: "
                                 "device %r, oracle %r; the lane's logits span %g .. %g, sample 0: %s"
                                 % (what, name, int(bad.sum()), b, pr, cell // c.lw, cell % c.lw, col, got[b, n, col], r[b, n, col],
                                    lane.min(), lane.max(), np.array2string(lane[0], precision=4, max_line_width=400)))
    rep64 = assert_rows_close(got, ref["z64"], v, what + " vs the float64 oracle", C=c.C, allowed=allowance(ref["floor"]))
    rep32 = assert_rows_close(got, ref["z32"], v, what + " vs the float32 oracle", C=c.C, allowed=allowance(ref["floor"], "float32"))
    return {"f64": rep64, "f32": rep32, "det": det}


def worst(rep):
    """Largest distance of a rows_report, ids left out (they are exact or wrong), in units of the bound."""
    return max([v["worst_in_bounds"] for k, v in rep.items() if k != "ids"] + [0.0])


# ---------------------------------------------------------------------------------------------
# the stage restated in float64 numpy, with one switch per wrong kernel
# ---------------------------------------------------------------------------------------------
MUTATIONS = {
    "drop_last_sample": "the last of the T samples is missing from every sum (the divisor stays T)",
    "bessel": "1 / (T - 1) in place of 1 / T",
    "swap_col_row": "column and row exchanged in the grid offset of a non-square grid",
    "swap_prior_hw": "ph and pw exchanged",
    "cell_major": "rows in cell-major order (cell * 3 + prior) instead of prior-major",
    "softmax_minus_one": "class slot C - 1 masked out of the softmax (max, sum and store)",
    "entropy_minus_one": "class slot C - 1 masked out of the entropy sums only",
    "swap_triangle": "cov[0][3] and cov[1][2] read each other's entry of the upper triangle s_ll[q]",
    "mi_swapped": "mutual information with its two terms exchanged",
    "box_base_plus_one": "the layer's block one row late",
}


def applies(mut, c):
    """Whether the wrong kernel `mut` computes anything different on case `c` at all."""
    if mut in ("drop_last_sample", "bessel"):
        return c.kind == 2 and c.T > 1
    if mut in ("swap_triangle", "mi_swapped"):
        return c.kind == 2
    if mut == "softmax_minus_one":
        return c.C > 1
    if mut == "entropy_minus_one":
        return c.kind > 0 and c.C > 1
    return True


def _xlogx_sum(p, n):
    return -np.sum(p[..., :n] * np.log(p[..., :n]), axis=-1)


def _logistic_entropy(s):
    return -((1 - s) * np.log(1 - s) + s * np.log(s))


def restate(c, raw, mut=None):
    """The buffer [B, n_total, D] (float32, sentinel outside the block) that a kernel with the fault `mut` (a key of MUTATIONS;
    None: the right kernel) writes for the float32 logits `raw`, evaluated in float64."""
    assert mut is None or mut in MUTATIONS
    B, T, lh, lw, C = c.B, c.T, c.lh, c.lw, c.C
    _, blk, D = geometry(c)
    with np.errstate(all="ignore"):
        d = raw.astype(np.float64).reshape(B, T, lh, lw, 3, blk)
        sig = lambda x: 1.0 / (1.0 + np.exp(-x))
        cs = 5 if c.kind == 0 else 10
        Cs = C - 1 if mut == "softmax_minus_one" else C              # slots the softmax sees
        Ce = C - 1 if mut in ("softmax_minus_one", "entropy_minus_one") else C
        cl = d[..., cs:cs + C]
        e = np.exp(cl[..., :Cs] - cl[..., :Cs].max(-1, keepdims=True))
        p = np.zeros(cl.shape)
        p[..., :Cs] = e / e.sum(-1, keepdims=True)
        obj = sig(d[..., 4 if c.kind == 0 else 8])
        ph = np.array([q[0] for q in PRIORS])
        pw = np.array([q[1] for q in PRIORS])
        if mut == "swap_prior_hw":
            ph, pw = pw, ph
        col = np.arange(lw, dtype=np.float64)[None, None, :, None]
        row = np.arange(lh, dtype=np.float64)[None, :, None, None]
        if mut == "swap_col_row":
            col, row = row, col

        def corners(t):                                              # t [B, lh, lw, 3, 4] -> y0, x0, y1, x1
            x = (col + sig(t[..., 0])) / lw
            y = (row + sig(t[..., 1])) / lh
            w2 = np.exp(t[..., 2]) * pw / 2
            h2 = np.exp(t[..., 3]) * ph / 2
            return np.stack([y - h2, x - w2, y + h2, x + w2], -1)

        one = np.ones((B, lh, lw, 3, 1))
        ids = [c.layer_id * one, np.arange(3, dtype=np.float64)[None, None, None, :, None] * one]
        if c.kind == 0:
            rows = np.concatenate([corners(d[:, 0, ..., 0:4]), obj[:, 0, ..., None], p[:, 0]], -1)
        elif c.kind == 1:
            var = np.exp(d[:, 0, ..., 4:8])
            tot = ((var[..., 0] * var[..., 1]) * var[..., 2]) * var[..., 3]
            rows = np.concatenate([corners(d[:, 0, ..., 0:4]), var, tot[..., None], obj[:, 0, ..., None],
                                   _logistic_entropy(obj[:, 0])[..., None], p[:, 0], _xlogx_sum(p[:, 0], Ce)[..., None]] + ids, -1)
        else:
            Tn = T - 1 if mut == "drop_last_sample" else T
            div = float(T - 1) if mut == "bessel" else float(T)
            mean = lambda a: a[:, :Tn].sum(1) / div
            loc = d[..., 0:4]
            ev = mean(loc)
            m2 = mean(loc[..., :, None] * loc[..., None, :])
            if mut == "swap_triangle":
                m2 = m2.copy()
                a, b = m2[..., 0, 3].copy(), m2[..., 1, 2].copy()
                m2[..., 0, 3] = m2[..., 3, 0] = b
                m2[..., 1, 2] = m2[..., 2, 1] = a
            cov = m2 - ev[..., :, None] * ev[..., None, :]
            ale = mean(np.exp(d[..., 4:8]))
            om = mean(obj)
            oH, oHs = _logistic_entropy(om), mean(_logistic_entropy(obj))
            pm = mean(p)
            cH, cHs = _xlogx_sum(pm, Ce), mean(_xlogx_sum(p, Ce))
            oMI, cMI = (oHs - oH, cHs - cH) if mut == "mi_swapped" else (oH - oHs, cH - cHs)
            bad = ~np.isfinite(cov).all((-1, -2))
            det = np.where(bad, np.nan, np.linalg.det(np.where(bad[..., None, None], 0.0, cov)))
            rows = np.concatenate([corners(ev), np.diagonal(cov, axis1=-2, axis2=-1), ale, det[..., None], ale.sum(-1, keepdims=True),
                                   om[..., None], oMI[..., None], oH[..., None], pm, cMI[..., None], cH[..., None]] + ids, -1)
        assert rows.shape == (B, lh, lw, 3, D)
        if mut == "cell_major":
            rows = rows.reshape(B, lh * lw * 3, D)
        else:
            rows = rows.transpose(0, 3, 1, 2, 4).reshape(B, 3 * lh * lw, D)
        buf = np.full((B, n_total(c), D), SENTINEL, dtype=np.float32)
        base = c.box_base + (1 if mut == "box_base_plus_one" else 0)
        buf[:, base:base + n_rows(c)] = rows.astype(np.float32)
    return buf
