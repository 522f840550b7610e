// score_recal.hip -- post-hoc recalibration of the detection score from the row's uncertainties (the logistic map: Platt 1999, Guo et
// al. 2017; box-dependent covariates: Kueppers et al. 2020).  A table of float64 weights w[g][k] per group (one, or one per class)
// turns a kept row's score s = obj * cls[class] into s' = sigmoid(w . x), x the row's features.  include/byolo.h and INTEGRATION.md
// ("Score recalibration") hold the definitions; tests/_score_recal_ref.py restates them in numpy.
//
//   score_recal_kernel   the apply: one lane per kept row.  In place (byolo_forward, behind the NMS) it reads count on the device and
//                        writes the obj column and score [B, cap]; out of place (byolo_score_recal_apply) the workgroup first copies
//                        its 256 rows with consecutive lanes.  A group at the identity (0, 1, 0, ...) leaves its rows alone.
//   sr_features_kernel   the features of records (or rows) as float64 [n, K], the device functions of the apply
//   sr_fit_kernel        the fit: one workgroup of 256 lanes per segment -- standardise, Newton on the ridge-penalised mean NLL, fold
//                        back -- inside the one launch.  Every sum is the fixed sum of recal_common.h: lane t sums the terms j = t
//                        (mod 256) in ascending j, one lane per quantity then adds the 256 partial sums in ascending t (LDS).  No
//                        atomics, no dependence on which workgroup runs first: two runs give the same bytes.
//
// Compiled without contraction (build.py _EXACT_F32): every float64 operation below is one operation of the restatement.
#include <cfloat>
#include "byolo_internal.h"
#include "recal_common.h"

namespace byk {

static constexpr int SR_MAXK = BYOLO_SCORE_RECAL_MAX_K, SR_MAXG = BYOLO_SCORE_RECAL_MAX_GROUPS;
static_assert((size_t)SR_MAXG * SR_MAXK * sizeof(double) == BYOLO_SCORE_RECAL_TABLE_BYTES, "the device table: [80][8] weights");
static_assert(SR_MAXK == 8, "the fit's accumulators are laid out for 8 features");

__device__ __forceinline__ double sr_logit(float s) {
    const double sd = (double)s;
    double t = sd > 1e-7 ? sd : 1e-7;
    t = t < 1.0 - 1e-7 ? t : 1.0 - 1e-7;
    const double om = 1.0 - t;
    const double q = t / om;
    return log(q);
}
__device__ __forceinline__ double sr_log_height(float ymin, float ymax) {
    double h = (double)__fsub_rn(ymax, ymin);
    if (!(h > 1e-6 && h <= DBL_MAX)) h = 1e-6;
    return log(h);
}
__device__ __forceinline__ double sr_col(float v, int kind) {
    double u = (double)v;
    if (kind == BYOLO_SCORE_RECAL_F_COL_ID) return fabs(u) <= DBL_MAX ? u : 0.0;
    if (!(u > 1e-12 && u <= DBL_MAX)) u = 1e-12;
    return log(u);
}
__device__ __forceinline__ double sr_feature(int kind, int col, float s, const float* r, int ymin_col, int ymax_col) {
    if (kind == BYOLO_SCORE_RECAL_F_BIAS) return 1.0;
    if (kind == BYOLO_SCORE_RECAL_F_LOGIT) return sr_logit(s);
    if (kind == BYOLO_SCORE_RECAL_F_LOG_HEIGHT) return sr_log_height(r[ymin_col], r[ymax_col]);
    return sr_col(r[col], kind);
}

__global__ __launch_bounds__(256) void score_recal_kernel(ScoreRecalParams p) {
    const int64_t n = (int64_t)p.B * p.cap;
    const int64_t row0 = (int64_t)blockIdx.x * 256;
    recal_copy_rows(p, row0, n);                              // out of place: every column and the padding come along
    const int64_t i = row0 + threadIdx.x;
    if (i >= n) return;
    const int b = (int)(i / p.cap), k = (int)(i - (int64_t)b * p.cap);
    if (k >= p.count[2 * b]) { p.score[i] = 0.f; return; }
    const float* r = p.in + i * p.D;
    // class and score: the evaluation's rule (eval_kernels.hip ev_score); the first NaN class score wins, as np.argmax has it
    float best = r[p.cls_start];
    bool nan = best != best;
    int c = 0;
    for (int q = 1; q < p.C; ++q) {
        const float v = r[p.cls_start + q];
        if (nan) continue;
        if (v != v) { nan = true; best = v; c = q; }
        else if (v > best) { best = v; c = q; }
    }
    const float s = __fmul_rn(r[p.obj_idx], best);
    const double* w = p.tab + (size_t)(p.by_class ? c : 0) * SR_MAXK;
    bool identity = w[0] == 0.0 && w[1] == 1.0;
    for (int q = 2; q < p.K; ++q) identity = identity && w[q] == 0.0;
    if (s != s || identity || !(best > 0.f && best <= FLT_MAX)) { p.score[i] = s; return; }
    double a = 0.0;
    for (int q = 0; q < p.K; ++q) {
        const double x = sr_feature(p.feat_kind[q], p.feat_col[q], s, r, 0, 2);
        const double wx = w[q] * x;
        a = a + wx;
    }
    const double e = exp(-a);
    const double d = 1.0 + e;
    const double sp = 1.0 / d;
    const float sf = (float)sp;
    p.score[i] = sf;
    const double o = (double)sf / (double)best;
    p.out[i * p.D + p.obj_idx] = (float)o;
}

hipError_t launch_score_recal(const ScoreRecalParams& p, hipStream_t st) {
    const int64_t n = (int64_t)p.B * p.cap;
    if (n < 1 || n >= (1ll << 31) * 256 || p.K < 2 || p.K > SR_MAXK || p.C < 1 || !p.in || !p.out || !p.count || !p.score || !p.tab) return hipErrorInvalidValue;
    if (p.obj_idx < 0 || p.obj_idx >= p.D || p.cls_start < 0 || p.cls_start + p.C > p.D || p.D < 4) return hipErrorInvalidValue;
    for (int k = 0; k < p.K; ++k)
        if (p.feat_kind[k] >= BYOLO_SCORE_RECAL_F_COL_ID && (p.feat_col[k] < 0 || p.feat_col[k] >= p.D)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(score_recal_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, p);
    return hipGetLastError();
}

// ---- the features of records ---------------------------------------------------------------------------------------------------
struct SrFeatParams {
    const float* src; int64_t n; int stride, score_col, ymin_col, ymax_col, K;
    int kind[8], col[8];
    double* x;               // [n, K]
};
__global__ __launch_bounds__(256) void sr_features_kernel(SrFeatParams p) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= p.n) return;
    const float* r = p.src + i * p.stride;
    const float s = r[p.score_col];
    for (int q = 0; q < p.K; ++q) p.x[i * p.K + q] = s != s ? recal_nan() : sr_feature(p.kind[q], p.col[q], s, r, p.ymin_col, p.ymax_col);
}

// ---- the fit ---------------------------------------------------------------------------------------------------------------------
struct SrFitParams {
    const double* x; const double* y; const int64_t* seg; int64_t n_total; int K; double l2; int64_t min_n;
    double* z;               // workspace [n, K]: the standardised features
    double* out;             // [n_seg][BYOLO_SCORE_RECAL_FIT_WORDS]
};

__device__ __forceinline__ double sr_softplus(double a) {
    const double m = fmax(a, 0.0);
    const double e = exp(-fabs(a));
    const double l = log1p(e);
    return m + l;
}
// a_j = sum_k u_k z_jk in ascending k, from 0.0 (u in LDS)
__device__ __forceinline__ double sr_dot(const double* u, const double* z, int K) {
    double a = 0.0;
    for (int k = 0; k < K; ++k) { const double t = u[k] * z[k]; a = a + t; }
    return a;
}
// the penalised mean loss at s_u (every lane returns it): fixed sum / n + (l2 / (2 n)) sum_{k >= 1} u_k^2
__device__ __forceinline__ double sr_loss(const SrFitParams& p, int64_t lo, int64_t hi, const double* s_u, double (*s_part)[256], double* s_tot, double dn) {
    double acc = 0.0;
    for (int64_t j = lo + threadIdx.x; j < hi; j += 256) {
        const double a = sr_dot(s_u, p.z + j * p.K, p.K);
        const double ya = p.y[j] * a;
        acc += sr_softplus(a) - ya;
    }
    recal_totals(s_part, s_tot, 5, acc, 0.0, 0.0, 0.0, 0.0);
    double pen = 0.0;
    for (int k = 1; k < p.K; ++k) { const double t = s_u[k] * s_u[k]; pen = pen + t; }
    const double c = p.l2 / (2.0 * dn);
    const double L = s_tot[0] / dn + c * pen;
    __syncthreads();                                         // s_tot is read; the next recal_totals may write it
    return L;
}
// mean NLL and mean Brier score of sigmoid(w . row) over the segment, rows of K doubles at `rows` (raw features) -- or, w == nullptr,
// of the identity: a = x_1
__device__ __forceinline__ void sr_nll_brier(const SrFitParams& p, int64_t lo, int64_t hi, const double* w, double (*s_part)[256], double* s_tot, double dn,
                                             double& nll, double& brier) {
    double an = 0.0, ab = 0.0;
    for (int64_t j = lo + threadIdx.x; j < hi; j += 256) {
        const double a = w ? sr_dot(w, p.x + j * p.K, p.K) : p.x[j * p.K + 1];
        const double y = p.y[j];
        const double ya = y * a;
        an += sr_softplus(a) - ya;
        const double e = exp(-a);
        const double d = 1.0 + e;
        const double pr = 1.0 / d;
        const double r = pr - y;
        ab += r * r;
    }
    recal_totals(s_part, s_tot, 5, an, ab, 0.0, 0.0, 0.0);
    nll = s_tot[0] / dn; brier = s_tot[1] / dn;
    __syncthreads();
}

__global__ __launch_bounds__(256) void sr_fit_kernel(SrFitParams p) {
    __shared__ double s_part[5][256];
    __shared__ double s_tot[45];                             // g [8], the upper Hessian [36] row by row, the loss
    __shared__ double s_u[8], s_try[8], s_d[8], s_g[8], s_w[8], s_mean[8], s_sd[8], s_y[8];
    __shared__ double s_H[8][8], s_L[8][8];
    __shared__ double s_state[4];                            // what the lanes do next, the loss at u, the last step, the step length
    __shared__ int s_drop[8];
    const int tid = threadIdx.x, K = p.K;
    int64_t lo, hi;
    recal_segment(p.seg, blockIdx.x, p.n_total, lo, hi);
    const int64_t n = hi - lo;
    double* out = p.out + (size_t)blockIdx.x * BYOLO_SCORE_RECAL_FIT_WORDS;
    const double nan = recal_nan();
    if (tid < 8) { s_u[tid] = 0.0; s_w[tid] = tid == 1 ? 1.0 : 0.0; s_mean[tid] = 0.0; s_sd[tid] = 1.0; s_drop[tid] = 0; }
    if (tid < 4) s_state[tid] = 0.0;
    __syncthreads();
    if (n == 0) {
        if (tid == 0) {
            out[0] = 0.0; out[1] = 0.0; out[2] = (double)BYOLO_SCORE_RECAL_EMPTY; out[3] = 0.0; out[4] = 1.0;
            out[5] = nan; out[6] = nan; out[7] = nan; out[8] = nan; out[9] = 0.0; out[10] = 0.0; out[11] = 0.0;
            for (int k = 0; k < 8; ++k) { out[12 + k] = k == 1 ? 1.0 : 0.0; out[20 + k] = 0.0; out[28 + k] = 1.0; }
        }
        return;
    }
    const double dn = (double)n;
    // the positives (an integer: exact in any order, summed in the fixed one all the same)
    double ytp = 0.0;
    for (int64_t j = lo + tid; j < hi; j += 256) { ytp += p.y[j]; p.z[j * K] = 1.0; }
    recal_totals(s_part, s_tot, 5, ytp, 0.0, 0.0, 0.0, 0.0);
    const double n_tp = s_tot[0];
    __syncthreads();
    // standardise: per feature the mean, then the population standard deviation; z = (x - mean) / sd, 0 for a dropped feature
    for (int k = 1; k < K; ++k) {
        double sx = 0.0;
        for (int64_t j = lo + tid; j < hi; j += 256) sx += p.x[j * K + k];
        recal_totals(s_part, s_tot, 5, sx, 0.0, 0.0, 0.0, 0.0);
        const double mean = s_tot[0] / dn;
        __syncthreads();
        double sv = 0.0;
        for (int64_t j = lo + tid; j < hi; j += 256) { const double d = p.x[j * K + k] - mean; sv += d * d; }
        recal_totals(s_part, s_tot, 5, sv, 0.0, 0.0, 0.0, 0.0);
        const double var = s_tot[0] / dn;
        const double sd = sqrt(var);
        __syncthreads();
        const bool drop = !(sd > 0.0 && sd <= DBL_MAX);
        for (int64_t j = lo + tid; j < hi; j += 256) { const double d = p.x[j * K + k] - mean; p.z[j * K + k] = drop ? 0.0 : d / sd; }
        if (tid == 0) { s_mean[k] = mean; s_sd[k] = sd; s_drop[k] = drop ? 1 : 0; }
    }
    __syncthreads();                                         // z of this segment is written by the lanes that read it again: a lane reads its own rows only
    double nll_before, brier_before;
    sr_nll_brier(p, lo, hi, nullptr, s_part, s_tot, dn, nll_before, brier_before);
    int status = BYOLO_SCORE_RECAL_IDENTITY;
    double iterations = 0.0, converged = 1.0, last = 0.0, nll_after = nll_before, brier_after = brier_before;
    if (n >= p.min_n && n_tp > 0.0 && n_tp < dn) {
        status = BYOLO_SCORE_RECAL_FIT;
        converged = 0.0;
        for (int it = 1; it <= 50; ++it) {
            // the K + K (K + 1) / 2 + 1 sums at u in one pass; features beyond K count as 0
            double acc[45];
#pragma unroll
            for (int q = 0; q < 45; ++q) acc[q] = 0.0;
            for (int64_t j = lo + tid; j < hi; j += 256) {
                double z[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) z[k] = k < K ? p.z[j * K + k] : 0.0;
                double a = 0.0;
#pragma unroll
                for (int k = 0; k < 8; ++k) if (k < K) { const double t = s_u[k] * z[k]; a = a + t; }
                const double y = p.y[j];
                const double e = exp(-a);
                const double d = 1.0 + e;
                const double pr = 1.0 / d;
                const double r = pr - y;
                const double om = 1.0 - pr;
                const double v = pr * om;
                const double ya = y * a;
                acc[44] += sr_softplus(a) - ya;
                int q = 8;
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    acc[k] += r * z[k];
                    const double vz = v * z[k];
#pragma unroll
                    for (int l = k; l < 8; ++l) { acc[q] += vz * z[l]; ++q; }
                }
            }
#pragma unroll
            for (int c = 0; c < 9; ++c) recal_totals(s_part, s_tot + 5 * c, 5, acc[5 * c], acc[5 * c + 1], acc[5 * c + 2], acc[5 * c + 3], acc[5 * c + 4]);
            if (tid == 0) {                                  // the Newton step, one operation per line
                const double ln = p.l2 / dn;
                int q = 8;
                for (int k = 0; k < 8; ++k) {
                    s_g[k] = s_tot[k] / dn;
                    for (int l = k; l < 8; ++l) { const double hkl = s_tot[q] / dn; s_H[k][l] = hkl; s_H[l][k] = hkl; ++q; }
                }
                double pen = 0.0;
                for (int k = 1; k < K; ++k) { const double t = s_u[k] * s_u[k]; pen = pen + t; }
                const double c2 = p.l2 / (2.0 * dn);
                const double L = s_tot[44] / dn + c2 * pen;
                for (int k = 1; k < K; ++k) { s_g[k] = s_g[k] + ln * s_u[k]; s_H[k][k] = s_H[k][k] + ln; }
                for (int k = 1; k < K; ++k)
                    if (s_drop[k]) {
                        s_g[k] = 0.0;
                        for (int l = 0; l < K; ++l) { s_H[k][l] = 0.0; s_H[l][k] = 0.0; }
                        s_H[k][k] = 1.0;
                    }
                bool ok = true;                              // Cholesky H = L L', then the two triangular solves
                for (int i = 0; i < K && ok; ++i)
                    for (int j = 0; j <= i; ++j) {
                        double s = s_H[i][j];
                        for (int m = 0; m < j; ++m) { const double t = s_L[i][m] * s_L[j][m]; s = s - t; }
                        if (i == j) {
                            if (!(s > 0.0 && s <= DBL_MAX)) { ok = false; break; }
                            s_L[i][i] = sqrt(s);
                        } else s_L[i][j] = s / s_L[j][j];
                    }
                double next = 3.0;                           // 0 the full step and go on, 1 converged, 2 search along d, 3 stop
                if (ok) {
                    for (int i = 0; i < K; ++i) {
                        double s = s_g[i];
                        for (int m = 0; m < i; ++m) { const double t = s_L[i][m] * s_y[m]; s = s - t; }
                        s_y[i] = s / s_L[i][i];
                    }
                    for (int i = K - 1; i >= 0; --i) {
                        double s = s_y[i];
                        for (int m = i + 1; m < K; ++m) { const double t = s_L[m][i] * s_d[m]; s = s - t; }
                        s_d[i] = s / s_L[i][i];
                    }
                    double mx = 0.0, gd = 0.0;
                    bool finite = true;
                    for (int k = 0; k < K; ++k) { const double ad = fabs(s_d[k]); finite = finite && ad <= DBL_MAX; mx = ad > mx ? ad : mx; const double t = s_g[k] * s_d[k]; gd = gd + t; }
                    s_state[2] = mx;
                    s_state[3] = (double)it;
                    if (finite) {
                        const double lim = 1e-12 * (1.0 + fabs(L));
                        next = mx < 1e-10 ? 1.0 : (gd <= lim ? 0.0 : 2.0);
                        if (next != 2.0) for (int k = 0; k < K; ++k) s_u[k] = s_u[k] - s_d[k];
                    }
                }
                s_state[0] = next; s_state[1] = L;
            }
            __syncthreads();
            const double next = s_state[0], L = s_state[1];
            if (next != 3.0 || s_state[3] == (double)it) { last = s_state[2]; iterations = s_state[3]; }
            __syncthreads();                                 // s_state is read; lane 0 may write it again
            if (next == 3.0) break;
            if (next == 1.0) { converged = 1.0; break; }
            if (next == 0.0) continue;
            double t = 1.0;
            bool took = false;
            for (int hv = 0; hv < 31; ++hv) {                // the step, halved at most 30 times while the loss does not fall
                if (tid < K) { const double td = t * s_d[tid]; s_try[tid] = s_u[tid] - td; }
                __syncthreads();
                const double Lt = sr_loss(p, lo, hi, s_try, s_part, s_tot, dn);
                if (Lt < L) { took = true; break; }          // (uniform: every lane holds the same Lt)
                t = t * 0.5;
                __syncthreads();
            }
            if (!took) break;
            __syncthreads();
            if (tid < K) s_u[tid] = s_try[tid];
            __syncthreads();
        }
        if (tid == 0) {                                      // fold back to weights of the raw features
            double acc = 0.0;
            for (int k = 1; k < K; ++k) {
                s_w[k] = s_drop[k] ? 0.0 : s_u[k] / s_sd[k];
                const double t = s_w[k] * s_mean[k];
                acc = acc + t;
            }
            s_w[0] = s_u[0] - acc;
        }
        __syncthreads();
        sr_nll_brier(p, lo, hi, s_w, s_part, s_tot, dn, nll_after, brier_after);
    }
    if (tid == 0) {
        int mask = 0;
        for (int k = 1; k < K; ++k) mask |= s_drop[k] << k;
        out[0] = dn; out[1] = n_tp; out[2] = (double)status; out[3] = iterations; out[4] = converged; out[5] = nll_before; out[6] = nll_after;
        out[7] = brier_before; out[8] = brier_after; out[9] = last; out[10] = (double)mask; out[11] = 0.0;
        for (int k = 0; k < 8; ++k) { out[12 + k] = k < K ? s_w[k] : 0.0; out[20 + k] = s_mean[k]; out[28 + k] = s_sd[k]; }
    }
}

}  // namespace byk

// ------------------------------------------------------------------------------------------------
// C-ABI (include/byolo.h "score recalibration")
// ------------------------------------------------------------------------------------------------
static void sr_layout(int kind, int* fixed, int* obj, int* cls) {
    *fixed = kind == BYOLO_DET_STANDARD ? 5 : kind == BYOLO_DET_ALEATORIC ? 14 : 21;
    *obj = kind == BYOLO_DET_STANDARD ? 4 : kind == BYOLO_DET_ALEATORIC ? 9 : 14;
    *cls = kind == BYOLO_DET_STANDARD ? 5 : kind == BYOLO_DET_ALEATORIC ? 11 : 17;
}
static int32_t sr_check_cfg(byolo_t* h, const byolo_score_recal_cfg* c, const char* what, bool weights = true) {
    if (c->struct_bytes != (int32_t)sizeof *c) return fail(h, BYOLO_ERR_ARG, "%s: struct_bytes %d, this library's byolo_score_recal_cfg has %d (include/byolo.h)", what, c->struct_bytes, (int)sizeof *c);
    if (c->kind != BYOLO_DET_STANDARD && c->kind != BYOLO_DET_ALEATORIC && c->kind != BYOLO_DET_EPISTEMIC) return fail(h, BYOLO_ERR_ARG, "%s: unknown kind %d (BYOLO_DET_*)", what, c->kind);
    if (c->by != BYOLO_SCORE_RECAL_BY_ALL && c->by != BYOLO_SCORE_RECAL_BY_CLASS) return fail(h, BYOLO_ERR_ARG, "%s: unknown by %d (BYOLO_SCORE_RECAL_BY_*)", what, c->by);
    if (c->cls_cnt < 1 || (c->by == BYOLO_SCORE_RECAL_BY_CLASS && c->cls_cnt > BYOLO_SCORE_RECAL_MAX_GROUPS))
        return fail(h, BYOLO_ERR_ARG, "%s: cls_cnt %d outside 1 .. %d groups of by = class", what, c->cls_cnt, BYOLO_SCORE_RECAL_MAX_GROUPS);
    if (c->K < 2 || c->K > BYOLO_SCORE_RECAL_MAX_K) return fail(h, BYOLO_ERR_ARG, "%s: K %d outside 2 .. %d (the bias and the logit are always there)", what, c->K, BYOLO_SCORE_RECAL_MAX_K);
    if (c->feat_kind[0] != BYOLO_SCORE_RECAL_F_BIAS || c->feat_kind[1] != BYOLO_SCORE_RECAL_F_LOGIT) return fail(h, BYOLO_ERR_ARG, "%s: feat_kind[0] / [1] are the bias and the logit", what);
    int fixed, obj, cls; sr_layout(c->kind, &fixed, &obj, &cls);
    for (int k = 2; k < c->K; ++k) {
        if (c->feat_kind[k] < BYOLO_SCORE_RECAL_F_LOG_HEIGHT || c->feat_kind[k] > BYOLO_SCORE_RECAL_F_COL_LOG) return fail(h, BYOLO_ERR_ARG, "%s: feat_kind[%d] = %d is not a feature (BYOLO_SCORE_RECAL_F_*)", what, k, c->feat_kind[k]);
        if (c->feat_kind[k] >= BYOLO_SCORE_RECAL_F_COL_ID && (c->feat_col[k] < 0 || c->feat_col[k] >= fixed + c->cls_cnt))
            return fail(h, BYOLO_ERR_ARG, "%s: feat_col[%d] = %d is outside the row of %d columns", what, k, c->feat_col[k], fixed + c->cls_cnt);
    }
    if (weights) {
        const int G = c->by == BYOLO_SCORE_RECAL_BY_CLASS ? c->cls_cnt : 1;
        for (int g = 0; g < G; ++g)
            for (int k = 0; k < c->K; ++k)
                if (!(fabs(c->w[g][k]) <= DBL_MAX)) return fail(h, BYOLO_ERR_ARG, "%s: w[%d][%d] = %g must be finite", what, g, k, c->w[g][k]);
    }
    return BYOLO_OK;
}
// the device layout: [80][8] weights; the identity outside the groups and the features
static void sr_pack(const byolo_score_recal_cfg* c, double* tab) {
    const int G = c->by == BYOLO_SCORE_RECAL_BY_CLASS ? c->cls_cnt : 1;
    for (int g = 0; g < BYOLO_SCORE_RECAL_MAX_GROUPS; ++g)
        for (int k = 0; k < BYOLO_SCORE_RECAL_MAX_K; ++k)
            tab[g * BYOLO_SCORE_RECAL_MAX_K + k] = g < G && k < c->K ? c->w[g][k] : (k == 1 ? 1.0 : 0.0);
}
static void sr_params(const byolo_score_recal_cfg& c, ScoreRecalParams* p) {
    memset(p, 0, sizeof *p);
    int fixed; sr_layout(c.kind, &fixed, &p->obj_idx, &p->cls_start);
    p->D = fixed + c.cls_cnt; p->C = c.cls_cnt; p->by_class = c.by == BYOLO_SCORE_RECAL_BY_CLASS; p->K = c.K;
    for (int k = 0; k < c.K; ++k) { p->feat_kind[k] = c.feat_kind[k]; p->feat_col[k] = c.feat_col[k]; }
}

extern "C" int32_t byolo_score_recal_table(const byolo_score_recal_cfg* cfg, double* h_table) {
    const char* what = "byolo_score_recal_table";
    if (!cfg || !h_table) return fail(nullptr, BYOLO_ERR_ARG, "%s: null argument", what);
    int32_t rc = sr_check_cfg(nullptr, cfg, what); if (rc) return rc;
    sr_pack(cfg, h_table);
    return BYOLO_OK;
}

// No copy from host memory in here (byolo_var_recal_apply says why): the caller brings the table to the device once and hands it in.
extern "C" int32_t byolo_score_recal_apply(const byolo_score_recal_cfg* cfg, const float* d_rows_in, const int32_t* d_count, int32_t B,
                                           int32_t cap, int32_t D, float* d_rows_out, float* d_score, const void* d_table, void* stream) {
    const char* what = "byolo_score_recal_apply";
    if (!cfg || !d_rows_in || !d_count || !d_rows_out || !d_score || !d_table) return fail(nullptr, BYOLO_ERR_ARG, "%s: null argument", what);
    int32_t rc = sr_check_cfg(nullptr, cfg, what); if (rc) return rc;
    ScoreRecalParams p;
    sr_params(*cfg, &p);
    if (D != p.D) return fail(nullptr, BYOLO_ERR_ARG, "%s: D %d: rows of kind %d with %d classes have %d columns", what, D, cfg->kind, cfg->cls_cnt, p.D);
    if (B < 0 || cap < 0 || (int64_t)B * cap >= (1ll << 31) * 256) return fail(nullptr, BYOLO_ERR_ARG, "%s: B %d, cap %d outside the launch", what, B, cap);
    if (reinterpret_cast<uintptr_t>(d_table) & 7) return fail(nullptr, BYOLO_ERR_ARG, "%s: d_table is not 8-byte aligned", what);
    const size_t bytes = (size_t)B * cap * D * sizeof(float), sbytes = (size_t)B * cap * sizeof(float);
    if (ranges_overlap(d_rows_in, bytes, d_rows_out, bytes)) return fail(nullptr, BYOLO_ERR_ARG, "%s: d_rows_out overlaps d_rows_in (the stand-alone stage never works in place)", what);
    if (ranges_overlap(d_rows_in, bytes, d_score, sbytes) || ranges_overlap(d_rows_out, bytes, d_score, sbytes)) return fail(nullptr, BYOLO_ERR_ARG, "%s: d_score overlaps the rows", what);
    if ((int64_t)B * cap == 0) return BYOLO_OK;
    p.in = d_rows_in; p.out = d_rows_out; p.count = d_count; p.score = d_score; p.B = B; p.cap = cap; p.tab = static_cast<const double*>(d_table);
    HIPCHK(nullptr, launch_score_recal(p, reinterpret_cast<hipStream_t>(stream)));
    return BYOLO_OK;
}

void byolo_score_recal_from_handle(const byolo_t* h, ScoreRecalParams* p) {
    sr_params(h->sr_cfg, p);
    p->D = h->row_len; p->obj_idx = h->obj_idx; p->cls_start = h->cls_start; p->tab = h->sr.dev;
}
void byolo_score_recal_pack(const byolo_t* h, double* tab) { sr_pack(&h->sr_cfg, tab); }

extern "C" int32_t byolo_set_score_recal(byolo_t* h, const byolo_score_recal_cfg* cfg) {
    const char* what = "byolo_set_score_recal";
    if (!h) return fail(nullptr, BYOLO_ERR_ARG, "%s: null handle", what);
    if (cfg) {
        int32_t rc = sr_check_cfg(h, cfg, what); if (rc) return rc;
        if (!h->n_det) return fail(h, BYOLO_ERR_STATE, "%s: add the detection layers first (the table is checked against them)", what);
        int kind = -1;
        for (const Layer& l : h->layers) if (l.op == OP_DETECTION) kind = l.det_kind;
        if (cfg->kind != kind) return fail(h, BYOLO_ERR_ARG, "%s: kind %d, the handle's detection layers are of kind %d", what, cfg->kind, kind);
        if (cfg->cls_cnt != h->cfg.cls_cnt) return fail(h, BYOLO_ERR_ARG, "%s: cls_cnt %d, the handle has %d classes", what, cfg->cls_cnt, h->cfg.cls_cnt);
        ScoreRecalParams p;
        sr_params(*cfg, &p);
        if (p.D != h->row_len || p.obj_idx != h->obj_idx || p.cls_start != h->cls_start) return fail(h, BYOLO_ERR_ARG, "%s: kind %d: the handle's rows have another layout", what, cfg->kind);
        h->sr_cfg = *cfg;
        h->sr.dirty = true;
    }
    h->sr.on = cfg != nullptr;
    side_out_forget(&h->out_score);
    // a captured forward holds the launches of the old setting, and the plan has score [B, cap] only while this is on (as byolo_set_box_vote)
    invalidate_plan(h);
    return BYOLO_OK;
}

extern "C" int32_t byolo_score_recal_scores(byolo_t* h, float* d_score, int32_t B, int32_t cap, void* stream) {
    if (!h || !d_score) return fail(h, BYOLO_ERR_ARG, "byolo_score_recal_scores: null argument");
    if (!h->out_score.ptr) return fail(h, BYOLO_ERR_STATE, "byolo_score_recal_scores: no byolo_forward with score recalibration (byolo_set_score_recal) and d_rows has run on this handle");
    return side_out_copy(h, &h->out_score, d_score, B, cap, "byolo_score_recal_scores", stream);
}

extern "C" int32_t byolo_score_recal_features(const byolo_score_recal_cfg* cfg, const float* d_src, int64_t n, int32_t stride, int32_t score_col,
                                              int32_t ymin_col, int32_t ymax_col, const int32_t* cols, double* d_x, void* stream) {
    const char* what = "byolo_score_recal_features";
    if (!cfg || !cols || (n > 0 && (!d_src || !d_x))) return fail(nullptr, BYOLO_ERR_ARG, "%s: null argument", what);
    int32_t rc = sr_check_cfg(nullptr, cfg, what, false); if (rc) return rc;
    if (n < 0 || n >= (1ll << 31) * 256 || stride < 1) return fail(nullptr, BYOLO_ERR_ARG, "%s: n %lld, stride %d", what, (long long)n, stride);
    if (score_col < 0 || score_col >= stride) return fail(nullptr, BYOLO_ERR_ARG, "%s: score_col %d outside the stride %d", what, score_col, stride);
    byk::SrFeatParams p; memset(&p, 0, sizeof p);
    p.src = d_src; p.n = n; p.stride = stride; p.score_col = score_col; p.ymin_col = ymin_col; p.ymax_col = ymax_col; p.K = cfg->K; p.x = d_x;
    for (int k = 0; k < cfg->K; ++k) {
        p.kind[k] = cfg->feat_kind[k]; p.col[k] = cols[k];
        if (p.kind[k] >= BYOLO_SCORE_RECAL_F_COL_ID && (cols[k] < 0 || cols[k] >= stride)) return fail(nullptr, BYOLO_ERR_ARG, "%s: cols[%d] = %d outside the stride %d", what, k, cols[k], stride);
        if (p.kind[k] == BYOLO_SCORE_RECAL_F_LOG_HEIGHT && (ymin_col < 0 || ymin_col >= stride || ymax_col < 0 || ymax_col >= stride))
            return fail(nullptr, BYOLO_ERR_ARG, "%s: ymin_col %d / ymax_col %d outside the stride %d", what, ymin_col, ymax_col, stride);
    }
    if (n == 0) return BYOLO_OK;
    hipLaunchKernelGGL(byk::sr_features_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), p);
    HIPCHK(nullptr, hipGetLastError());
    return BYOLO_OK;
}

extern "C" size_t byolo_score_recal_fit_workspace_bytes(int64_t n, int32_t K) { return n < 1 || K < 1 ? 0 : (size_t)n * K * sizeof(double); }

extern "C" int32_t byolo_score_recal_fit(const double* d_x, const double* d_y, const int64_t* d_seg, int32_t n_seg, int64_t n, int32_t K,
                                         double l2, int64_t min_n, double* d_out, void* d_ws, size_t ws_bytes, void* stream) {
    const char* what = "byolo_score_recal_fit";
    int32_t rc = byolo_recal_check_fit(what, d_seg && d_out && (n <= 0 || (d_x && d_y && d_ws)), n_seg, n, d_ws, ws_bytes, byolo_score_recal_fit_workspace_bytes(n, K),
                                       "byolo_score_recal_fit_workspace_bytes(n, K)");
    if (rc) return rc;
    if (K < 2 || K > BYOLO_SCORE_RECAL_MAX_K) return fail(nullptr, BYOLO_ERR_ARG, "%s: K %d outside 2 .. %d", what, K, BYOLO_SCORE_RECAL_MAX_K);
    if (!(l2 >= 0.0 && l2 <= DBL_MAX)) return fail(nullptr, BYOLO_ERR_ARG, "%s: l2 %g must be >= 0 and finite", what, l2);
    if (min_n < 1) return fail(nullptr, BYOLO_ERR_ARG, "%s: min_n %lld must be >= 1", what, (long long)min_n);
    byk::SrFitParams p;
    p.x = d_x; p.y = d_y; p.seg = d_seg; p.n_total = n; p.K = K; p.l2 = l2; p.min_n = min_n; p.z = static_cast<double*>(d_ws); p.out = d_out;
    hipLaunchKernelGGL(byk::sr_fit_kernel, dim3((unsigned)n_seg), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), p);
    HIPCHK(nullptr, hipGetLastError());
    return BYOLO_OK;
}
