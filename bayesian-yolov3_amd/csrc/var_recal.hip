// var_recal.hip -- post-hoc recalibration of the predicted variances (sigma-scaling: Laves et al. 2020; for detectors: Feng et al.
// 2019; in general: Kuleshov et al. 2018).  A table of float64 pairs (a, b) per detection layer, prior and coordinate turns a row's
// variance v into v' = a v^b.  include/byolo.h and INTEGRATION.md ("Variance recalibration") hold the definitions;
// tests/_var_recal_ref.py restates them in numpy.
//
//   var_recal_kernel   the apply: one lane per row.  In place (byolo_forward, behind the decode) it reads the two id columns and the
//                      4 or 8 variance columns of a row and writes those and the 1 or 2 columns derived from them; out of place
//                      (byolo_var_recal_apply) the workgroup first copies its 256 rows with consecutive lanes.  b == 1 is one
//                      float64 multiply per column -- no exp, no log: bit-exact against numpy.
//   vr_fit_kernel      the fit: one workgroup of 256 lanes per segment (a group and coordinate), the whole Newton iteration of the
//                      power method inside the one launch.  Lane t sums the terms j = t (mod 256) in ascending j; lanes 0 .. 4
//                      then each add the 256 partial sums of one quantity in ascending t (LDS; recal_common.h).  No atomics, no
//                      dependence on which workgroup runs first: two runs give the same bytes.
//
// Compiled without contraction (build.py _EXACT_F32): every float64 operation below is one operation of the restatement.
#include <cfloat>
#include "byolo_internal.h"
#include "recal_common.h"

namespace byk {

static constexpr int VR_MAXL = BYOLO_EVAL_LOC_MAX_LAYERS, VR_MAXP = BYOLO_EVAL_LOC_MAX_PRIORS;
static_assert((size_t)VR_MAXL * VR_MAXP * 4 * 2 * sizeof(double) == BYOLO_VAR_RECAL_TABLE_BYTES, "the device table: [8][16][4] pairs (a, b)");
static constexpr double VR_TWO_PI = 6.283185307179586;

// a layer / prior id: finite, integral, inside [0, n)
__device__ __forceinline__ bool vr_id(float v, int n, int& out) {
    const bool ok = v >= 0.f && v < (float)n && floorf(v) == v;
    out = ok ? (int)v : 0;
    return ok;
}
// the factor f = v' / v of one coordinate; false: the coordinate stays as it is
__device__ __forceinline__ bool vr_factor(double a, double b, double v, double& f) {
    f = 1.0;
    if (b == 1.0) { f = a; return true; }
    if (!(v > 0.0) || !(v <= DBL_MAX)) return false;
    const double lv = log(v);
    const double e = (b - 1.0) * lv;
    const double x = exp(e);
    f = a * x;
    return true;
}
__device__ __forceinline__ float vr_scale(float col, double f) {      // rounded once; a NaN keeps its bits
    if (col != col) return col;
    const double d = (double)col * f;
    return (float)d;
}
__device__ __forceinline__ bool vr_same(float x, float y) { return __float_as_uint(x) == __float_as_uint(y); }

__global__ __launch_bounds__(256) void var_recal_kernel(VarRecalParams p) {
    const int64_t row0 = (int64_t)blockIdx.x * 256;
    recal_copy_rows(p, row0, p.n);                            // out of place: every column comes along
    const int64_t i = row0 + threadIdx.x;
    if (i >= p.n) return;
    const float* r = p.in + i * p.D;
    float* o = p.out + i * p.D;
    int layer = 0, prior = 0;
    if (!vr_id(r[p.D - 2], p.n_layers, layer)) return;
    if (!vr_id(r[p.D - 1], p.n_priors[layer], prior)) return;
    const double* t = p.tab + (size_t)(layer * VR_MAXP + prior) * 8;
    if (p.kind == BYOLO_DET_ALEATORIC) {
        float c[4];
        bool changed = false;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float col = r[4 + k];
            double f;
            c[k] = vr_factor(t[2 * k], t[2 * k + 1], (double)col, f) ? vr_scale(col, f) : col;
            changed = changed || !vr_same(c[k], col);
            o[4 + k] = c[k];
        }
        if (changed) o[8] = ((c[0] * c[1]) * c[2]) * c[3];   // tf.reduce_prod, as decode_ale_kernel forms it
        return;
    }
    float ev[4], av[4];
    double fe[4];
    bool ale_changed = false;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float e0 = r[4 + k], a0 = r[8 + k];
        const double v = p.target == BYOLO_VAR_RECAL_ALE ? (double)a0 : p.target == BYOLO_VAR_RECAL_EPI ? (double)e0 : (double)e0 + (double)a0;
        double f;
        const bool on = vr_factor(t[2 * k], t[2 * k + 1], v, f);
        ev[k] = e0; av[k] = a0; fe[k] = 1.0;
        if (on && p.target != BYOLO_VAR_RECAL_ALE) { ev[k] = vr_scale(e0, f); fe[k] = f; }
        if (on && p.target != BYOLO_VAR_RECAL_EPI) av[k] = vr_scale(a0, f);
        ale_changed = ale_changed || !vr_same(av[k], a0);
        o[4 + k] = ev[k]; o[8 + k] = av[k];
    }
    if (p.target != BYOLO_VAR_RECAL_ALE) {                   // det(S C S) = det(C) prod s^2: the determinant of the scaled covariance
        const double P = ((fe[0] * fe[1]) * fe[2]) * fe[3];
        o[12] = vr_scale(r[12], P);
    }
    if (ale_changed) o[13] = (((0.f + av[0]) + av[1]) + av[2]) + av[3];      // as decode_epi_kernel forms it
}

hipError_t launch_var_recal(const VarRecalParams& p, hipStream_t st) {
    if (p.n < 1 || p.n >= (1ll << 31) * 256 || p.D < 14 || !p.in || !p.out || !p.tab) return hipErrorInvalidValue;
    hipLaunchKernelGGL(var_recal_kernel, dim3((unsigned)((p.n + 255) / 256)), dim3(256), 0, st, p);
    return hipGetLastError();
}

// ---- the fit ---------------------------------------------------------------------------------------------------------------------
struct VrFitParams {
    const double* r; const double* v; const int64_t* seg; int64_t n_total; int method;
    double* lv;              // workspace [n]: log v
    double* out;             // [n_seg][BYOLO_VAR_RECAL_FIT_WORDS]
};

// 0.5 (log(2 pi v) + r^2 / v), one operation per line (byolo/eval_loc.py nll_terms with z^2 = r^2 / v)
__device__ __forceinline__ double vr_nll(double r2, double v) {
    const double a = VR_TWO_PI * v;
    const double l = log(a);
    const double q = r2 / v;
    const double s = l + q;
    return 0.5 * s;
}

__global__ __launch_bounds__(256) void vr_fit_kernel(VrFitParams p) {
    __shared__ double s_part[5][256];
    __shared__ double s_tot[5];
    __shared__ double s_state[4];                            // alpha, b, what the lanes do next, iterations
    const int tid = threadIdx.x;
    int64_t lo, hi;
    recal_segment(p.seg, blockIdx.x, p.n_total, lo, hi);
    const int64_t n = hi - lo;
    double* out = p.out + (size_t)blockIdx.x * BYOLO_VAR_RECAL_FIT_WORDS;
    const double nan = recal_nan();
    if (n == 0) {
        if (tid == 0) { out[0] = 0.0; out[1] = 1.0; out[2] = 1.0; out[3] = nan; out[4] = nan; out[5] = nan; out[6] = 0.0; out[7] = (double)BYOLO_VAR_RECAL_EMPTY; out[8] = 1.0; out[9] = 0.0; }
        return;
    }
    const double dn = (double)n;
    // pass 1: sum r^2 / v, sum log v, the NLL as it stands; log v is kept for the passes behind this one
    double q_sum = 0.0, l_sum = 0.0, nll_sum = 0.0;
    for (int64_t j = lo + tid; j < hi; j += 256) {
        const double r = p.r[j], v = p.v[j];
        const double r2 = r * r;
        const double q = r2 / v;
        const double lv = log(v);
        p.lv[j] = lv;
        q_sum += q; l_sum += lv; nll_sum += vr_nll(r2, v);
    }
    recal_totals(s_part, s_tot, 3, q_sum, l_sum, nll_sum, 0.0, 0.0);
    const double S = s_tot[0];
    const double a_scale = S / dn, ubar = s_tot[1] / dn, nll_before = s_tot[2] / dn;
    __syncthreads();                                         // s_tot is read; the next recal_totals may write it
    int status = BYOLO_VAR_RECAL_FITTED;
    double a = a_scale, b = 1.0, U = 0.0, iterations = 0.0, converged = 1.0;
    if (!(S > 0.0) || !(S <= DBL_MAX)) { status = BYOLO_VAR_RECAL_IDENTITY; a = 1.0; }
    else if (p.method == BYOLO_VAR_RECAL_POWER) {
        // U = max |u|: a maximum does not depend on the order
        double um = 0.0;
        for (int64_t j = lo + tid; j < hi; j += 256) { const double u = p.lv[j] - ubar; um = fmax(um, fabs(u)); }
        s_part[0][tid] = um;
        __syncthreads();
        if (tid == 0) { double m = 0.0; for (int t = 0; t < 256; ++t) m = fmax(m, s_part[0][t]); s_tot[0] = m; }
        __syncthreads();
        U = s_tot[0];
        __syncthreads();
        if (n < 3) status = BYOLO_VAR_RECAL_SCALE_FALLBACK;
        else {
            double alpha = log(a_scale);
            converged = 0.0;
            for (int it = 1; it <= 100; ++it) {
                double g0 = 0.0, g1 = 0.0, h00 = 0.0, h01 = 0.0, h11 = 0.0;
                for (int64_t j = lo + tid; j < hi; j += 256) {
                    const double r = p.r[j];
                    const double r2 = r * r;
                    const double u = p.lv[j] - ubar;
                    const double bu = b * u;
                    const double au = alpha + ubar;
                    const double eta = au + bu;
                    const double x = exp(-eta);
                    const double w = r2 * x;
                    const double d = 1.0 - w;
                    const double ud = u * d;
                    const double wu = w * u;
                    const double wuu = wu * u;
                    g0 += d; g1 += ud; h00 += w; h01 += wu; h11 += wuu;
                }
                recal_totals(s_part, s_tot, 5, g0, g1, h00, h01, h11);
                if (tid == 0) {                              // the Newton step, one operation per line
                    const double G0 = s_tot[0], G1 = s_tot[1], H00 = s_tot[2], H01 = s_tot[3], H11 = s_tot[4];
                    const double hh = H00 * H11;
                    const double oo = H01 * H01;
                    const double det = hh - oo;
                    const double lim = 1e-12 * hh;
                    double next = 0.0;                       // 0 go on, 1 converged, 2 the scale answer
                    if (!(det > lim)) next = 2.0;
                    else {
                        const double n0 = H11 * G0;
                        const double n1 = H01 * G1;
                        const double m0 = H00 * G1;
                        const double m1 = H01 * G0;
                        const double da = -((n0 - n1) / det);
                        const double db = -((m0 - m1) / det);
                        const double sb = fabs(db) * U;
                        const double size = fabs(da) + sb;
                        if (!(size <= DBL_MAX)) next = 2.0;
                        else {
                            const double k = size > 1.0 ? 1.0 / size : 1.0;
                            const double sa = da * k;
                            const double sbb = db * k;
                            s_state[0] = alpha + sa;
                            s_state[1] = b + sbb;
                            s_state[3] = (double)it;
                            if (size <= 1e-10) next = 1.0;
                        }
                    }
                    s_state[2] = next;
                }
                __syncthreads();
                const double next = s_state[2];
                if (next != 2.0) { alpha = s_state[0]; b = s_state[1]; iterations = s_state[3]; }
                __syncthreads();                             // s_state and s_tot are read; the next round may write them
                if (next == 2.0) { status = BYOLO_VAR_RECAL_SCALE_FALLBACK; break; }
                if (next == 1.0) { converged = 1.0; break; }
            }
            if (status == BYOLO_VAR_RECAL_FITTED) {
                const double ob = 1.0 - b;
                const double e = ubar * ob;
                const double ae = alpha + e;
                a = exp(ae);
            } else { b = 1.0; converged = 1.0; }
        }
    }
    // the NLL at the fitted table: v' = a v (b == 1) or a exp(b log v)
    double after = 0.0;
    for (int64_t j = lo + tid; j < hi; j += 256) {
        const double r = p.r[j], v = p.v[j];
        const double r2 = r * r;
        double vp;
        if (b == 1.0) vp = a * v;
        else { const double bl = b * p.lv[j]; const double x = exp(bl); vp = a * x; }
        after += vr_nll(r2, vp);
    }
    recal_totals(s_part, s_tot, 1, after, 0.0, 0.0, 0.0, 0.0);
    if (tid == 0) {
        out[0] = dn; out[1] = a; out[2] = b; out[3] = a_scale; out[4] = nll_before; out[5] = s_tot[0] / dn;
        out[6] = iterations; out[7] = (double)status; out[8] = converged; out[9] = U;
    }
}

}  // namespace byk

// ------------------------------------------------------------------------------------------------
// C-ABI (include/byolo.h "variance recalibration")
// ------------------------------------------------------------------------------------------------
static int32_t vr_check_cfg(byolo_t* h, const byolo_var_recal_cfg* c, const char* what) {
    if (c->struct_bytes != (int32_t)sizeof *c) return fail(h, BYOLO_ERR_ARG, "%s: struct_bytes %d, this library's byolo_var_recal_cfg has %d (include/byolo.h)", what, c->struct_bytes, (int)sizeof *c);
    if (c->kind != BYOLO_DET_ALEATORIC && c->kind != BYOLO_DET_EPISTEMIC) return fail(h, BYOLO_ERR_ARG, "%s: kind %d is neither BYOLO_DET_ALEATORIC nor BYOLO_DET_EPISTEMIC (standard rows carry no variances)", what, c->kind);
    if (c->target < BYOLO_VAR_RECAL_ALE || c->target > BYOLO_VAR_RECAL_TOTAL) return fail(h, BYOLO_ERR_ARG, "%s: unknown target %d (BYOLO_VAR_RECAL_*)", what, c->target);
    if (c->kind == BYOLO_DET_ALEATORIC && c->target != BYOLO_VAR_RECAL_ALE) return fail(h, BYOLO_ERR_ARG, "%s: target %d needs epistemic variances, aleatoric rows have none", what, c->target);
    if (c->n_layers < 1 || c->n_layers > BYOLO_EVAL_LOC_MAX_LAYERS) return fail(h, BYOLO_ERR_ARG, "%s: n_layers %d outside 1 .. %d", what, c->n_layers, BYOLO_EVAL_LOC_MAX_LAYERS);
    for (int l = 0; l < c->n_layers; ++l) {
        if (c->n_priors[l] < 1 || c->n_priors[l] > BYOLO_EVAL_LOC_MAX_PRIORS) return fail(h, BYOLO_ERR_ARG, "%s: n_priors of layer %d outside 1 .. %d", what, l, BYOLO_EVAL_LOC_MAX_PRIORS);
        for (int p = 0; p < c->n_priors[l]; ++p)
            for (int k = 0; k < 4; ++k) {
                const double a = c->a[l][p][k], b = c->b[l][p][k];
                if (!(a > 0.0) || !(a <= DBL_MAX)) return fail(h, BYOLO_ERR_ARG, "%s: a[%d][%d][%d] = %g must be > 0 and finite", what, l, p, k, a);
                if (!(fabs(b) <= DBL_MAX)) return fail(h, BYOLO_ERR_ARG, "%s: b[%d][%d][%d] = %g must be finite", what, l, p, k, b);
            }
    }
    return BYOLO_OK;
}
// the device layout: [8][16][4] pairs (a, b); the identity outside the geometry
static void vr_pack(const byolo_var_recal_cfg* c, double* tab) {
    for (int l = 0; l < BYOLO_EVAL_LOC_MAX_LAYERS; ++l)
        for (int p = 0; p < BYOLO_EVAL_LOC_MAX_PRIORS; ++p)
            for (int k = 0; k < 4; ++k) {
                const bool in = l < c->n_layers && p < c->n_priors[l];
                double* e = tab + ((size_t)(l * BYOLO_EVAL_LOC_MAX_PRIORS + p) * 4 + k) * 2;
                e[0] = in ? c->a[l][p][k] : 1.0; e[1] = in ? c->b[l][p][k] : 1.0;
            }
}
static void vr_params(const byolo_var_recal_cfg& c, VarRecalParams* p) {
    memset(p, 0, sizeof *p);
    p->kind = c.kind; p->target = c.target; p->n_layers = c.n_layers;
    for (int l = 0; l < c.n_layers; ++l) p->n_priors[l] = c.n_priors[l];
}

extern "C" int32_t byolo_var_recal_table(const byolo_var_recal_cfg* cfg, double* h_table) {
    const char* what = "byolo_var_recal_table";
    if (!cfg || !h_table) return fail(nullptr, BYOLO_ERR_ARG, "%s: null argument", what);
    int32_t rc = vr_check_cfg(nullptr, cfg, what); if (rc) return rc;
    vr_pack(cfg, h_table);
    return BYOLO_OK;
}

// No copy from host memory in here: a table in memory of this call's own would have to outlive the call, and one copied on another
// stream than the launch's would have to be waited for.  The caller brings the table to the device once and hands it in.
extern "C" int32_t byolo_var_recal_apply(const byolo_var_recal_cfg* cfg, const float* d_in, int64_t n, int32_t D, float* d_out,
                                         const void* d_table, void* stream) {
    const char* what = "byolo_var_recal_apply";
    if (!cfg || !d_in || !d_out || !d_table) return fail(nullptr, BYOLO_ERR_ARG, "%s: null argument", what);
    int32_t rc = vr_check_cfg(nullptr, cfg, what); if (rc) return rc;
    const int32_t need = cfg->kind == BYOLO_DET_ALEATORIC ? 14 : 21;
    if (D < need) return fail(nullptr, BYOLO_ERR_ARG, "%s: D %d: rows of kind %d have at least %d columns", what, D, cfg->kind, need);
    if (n < 0 || n >= (1ll << 31) * 256) return fail(nullptr, BYOLO_ERR_ARG, "%s: n %lld outside the launch", what, (long long)n);
    if (reinterpret_cast<uintptr_t>(d_table) & 7) return fail(nullptr, BYOLO_ERR_ARG, "%s: d_table is not 8-byte aligned", what);
    const size_t bytes = (size_t)n * D * sizeof(float);
    if (ranges_overlap(d_in, bytes, d_out, bytes)) return fail(nullptr, BYOLO_ERR_ARG, "%s: d_out overlaps d_in (the stand-alone stage never works in place)", what);
    if (n == 0) return BYOLO_OK;
    VarRecalParams p;
    vr_params(*cfg, &p);
    p.in = d_in; p.out = d_out; p.n = n; p.D = D; p.tab = static_cast<const double*>(d_table);
    HIPCHK(nullptr, launch_var_recal(p, reinterpret_cast<hipStream_t>(stream)));
    return BYOLO_OK;
}

void byolo_var_recal_from_handle(const byolo_t* h, VarRecalParams* p) {
    vr_params(h->vr_cfg, p);
    p->D = h->row_len; p->tab = h->vr.dev;
}
void byolo_var_recal_pack(const byolo_t* h, double* tab) { vr_pack(&h->vr_cfg, tab); }

// The device table of either recalibration stage (score_recal.hip's as well) brought up to date, `pack` filling t->host first.
// The copy runs on the forward's own stream from memory the handle owns, and the stream is waited for: whatever stream the launch
// that reads the table is enqueued on afterwards -- a caller alternates forwards over several non-blocking streams, which nothing
// orders against the default stream -- the table is there.  (A synchronous copy on the default stream may return once the source is
// staged, before the bytes have landed.)
int32_t byolo_recal_upload(byolo_t* h, RecalTable* t, void (*pack)(const byolo_t* h, double* tab), hipStream_t st) {
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipDeviceSynchronize());                       // a forward in flight, or a graph replaying, may still read the table
    if (!t->dev) HIPCHK(h, hipMalloc(reinterpret_cast<void**>(&t->dev), t->bytes));
    pack(h, t->host);
    HIPCHK(h, hipMemcpyAsync(t->dev, t->host, t->bytes, hipMemcpyHostToDevice, st));
    HIPCHK(h, hipStreamSynchronize(st));
    t->dirty = false;
    return BYOLO_OK;
}

extern "C" int32_t byolo_set_var_recal(byolo_t* h, const byolo_var_recal_cfg* cfg) {
    const char* what = "byolo_set_var_recal";
    if (!h) return fail(nullptr, BYOLO_ERR_ARG, "%s: null handle", what);
    if (cfg) {
        int32_t rc = vr_check_cfg(h, cfg, what); if (rc) return rc;
        if (!h->n_det) return fail(h, BYOLO_ERR_STATE, "%s: add the detection layers first (the table is checked against them)", what);
        int kind = -1, n = 0;
        for (const Layer& l : h->layers) if (l.op == OP_DETECTION) { kind = l.det_kind; ++n; }
        if (cfg->kind != kind) return fail(h, BYOLO_ERR_ARG, "%s: kind %d, the handle's detection layers are of kind %d", what, cfg->kind, kind);
        if (cfg->n_layers != n) return fail(h, BYOLO_ERR_ARG, "%s: n_layers %d, the graph has %d detection layers", what, cfg->n_layers, n);
        int k = 0;
        for (const Layer& l : h->layers) {
            if (l.op != OP_DETECTION) continue;
            const int32_t have = (int32_t)(sizeof l.priors / sizeof l.priors[0] / 2);      // the (h, w) pairs the layer holds
            if (cfg->n_priors[k] != have) return fail(h, BYOLO_ERR_ARG, "%s: n_priors of layer %d is %d, the detection layer has %d priors", what, k, cfg->n_priors[k], have);
            ++k;
        }
        h->vr_cfg = *cfg;
        h->vr.dirty = true;
    }
    h->vr.on = cfg != nullptr;
    // a captured forward holds the launches of the old setting (as byolo_set_box_vote); the device table is brought up to date by the
    // next forward, behind a wait for the device, so a replay that is still running reads the table it was launched with
    invalidate_plan(h);
    return BYOLO_OK;
}

int32_t byolo_recal_check_fit(const char* what, bool have_ptrs, int32_t n_seg, int64_t n, const void* d_ws, size_t ws_bytes, size_t need, const char* ws_call) {
    if (!have_ptrs) return fail(nullptr, BYOLO_ERR_ARG, "%s: null argument", what);
    if (n_seg < 1 || n < 0) return fail(nullptr, BYOLO_ERR_ARG, "%s: n_seg %d, n %lld", what, n_seg, (long long)n);
    if (ws_bytes < need) return fail(nullptr, BYOLO_ERR_NOMEM, "%s: workspace %zu < %s = %zu", what, ws_bytes, ws_call, need);
    if (reinterpret_cast<uintptr_t>(d_ws) & 7) return fail(nullptr, BYOLO_ERR_ARG, "%s: d_ws is not 8-byte aligned", what);
    return BYOLO_OK;
}

extern "C" size_t byolo_var_recal_fit_workspace_bytes(int64_t n) { return n < 1 ? 0 : (size_t)n * sizeof(double); }

extern "C" int32_t byolo_var_recal_fit(const double* d_r, const double* d_v, const int64_t* d_seg, int32_t n_seg, int64_t n,
                                       int32_t method, double* d_out, void* d_ws, size_t ws_bytes, void* stream) {
    const char* what = "byolo_var_recal_fit";
    int32_t rc = byolo_recal_check_fit(what, d_seg && d_out && (n <= 0 || (d_r && d_v && d_ws)), n_seg, n, d_ws, ws_bytes, byolo_var_recal_fit_workspace_bytes(n),
                                       "byolo_var_recal_fit_workspace_bytes(n)");
    if (rc) return rc;
    if (method != BYOLO_VAR_RECAL_SCALE && method != BYOLO_VAR_RECAL_POWER) return fail(nullptr, BYOLO_ERR_ARG, "%s: unknown method %d (BYOLO_VAR_RECAL_SCALE / _POWER)", what, method);
    byk::VrFitParams p;
    p.r = d_r; p.v = d_v; p.seg = d_seg; p.n_total = n; p.method = method; p.lv = static_cast<double*>(d_ws); p.out = d_out;
    hipLaunchKernelGGL(byk::vr_fit_kernel, dim3((unsigned)n_seg), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), p);
    HIPCHK(nullptr, hipGetLastError());
    return BYOLO_OK;
}
