// box_vote.hip -- variance voting (He et al., "Bounding Box Regression with Uncertainty for Accurate Object Detection", CVPR 2019)
// behind the NMS: every kept row's box becomes the mean of the pre-NMS boxes of its class that overlap it, each weighted by an IoU
// kernel and by the inverse of its own predicted variance.  include/byolo.h and INTEGRATION.md ("Variance voting") hold the
// definition; tests/_box_vote_ref.py restates it in numpy.
//
//   bv_pack   once per batch, one lane per pre-NMS row: the row's class -- classify_row and score_key of nms_box.h, the functions
//             the NMS pipeline itself calls, evaluated AGAIN on the same rows (no coupling to the NMS workspace: the stage also
//             runs stand-alone, behind byolo_sort_nms) --, everything else that decides whether the row may vote at all (score,
//             finite box, ids, variances) folded into that byte (PC_NONE = never votes), the sorted float32 corners, and the four
//             1 / max(var_c, var_floor) as doubles.  Index-aligned SoA: the vote reads them with consecutive lanes.
//   bv_vote   a workgroup takes BV_KT = 16 kept rows of one image against the image's candidates in tiles of BV_TILE = 1024, corners and
//             class byte staged in LDS (17 KB).  16 lanes share a kept row: lane s visits the candidates j = s (mod 16) in ascending
//             order, so the four kept rows of a wave read the same LDS words (broadcast) and consecutive lanes consecutive words.
//             The float32 IoU rejects nearly every pair; only a voter costs float64 work (exp, 8 multiply-adds) and the read of
//             its four inverse variances from global memory.  FP64 runs at half the FP32 vector rate on this chip and voters
//             are a small share of the pairs, so the float32 test, not the float64 sum, bounds the kernel.
//
// The order of every sum is fixed: lane s of a kept row adds its candidates in ascending index, and the 16 partial sums are folded
// by a butterfly (xor 1, 2, 4, 8).  Nothing depends on which workgroup runs first, on atomics, or on the order pc_scatter left the
// class segments in; an image gives the same bytes at any position of any batch.  Eight double accumulators with compile-time
// names: no private segment (tests/test_no_scratch.py).  Nothing needs clearing: every vote_n word is written by the vote itself.
#include "byolo_internal.h"
#include "nms_box.h"

namespace byk {

static constexpr int BV_KT = 16;                             // kept rows per workgroup
static constexpr int BV_SUB = 16;                            // lanes per kept row
static constexpr int BV_TILE = 1024;                         // candidates per LDS tile (a multiple of BV_SUB)
static_assert(BV_KT * BV_SUB == 256 && BV_TILE % BV_SUB == 0, "bv_vote_kernel: 256 threads, whole strides per tile");

struct BvWs {
    double* g[4];                                            // [B][N] 1 / max(var_c, var_floor), c = cx, cy, w, h
    float *y0, *x0, *y1, *x1;                                // [B][N] corners as make_box sorts them
    unsigned char* cls;                                      // [B][N] class of a row that may vote, PC_NONE otherwise
};
static size_t bv_ws_layout(int B, int64_t N, char* base, BvWs* w) {
    size_t o = 0;
    auto take = [&](size_t bytes) { char* p = base ? base + o : nullptr; o += (bytes + 255) / 256 * 256; return p; };
    const size_t n = (size_t)B * (size_t)N;
    char* g[4]; for (int c = 0; c < 4; ++c) g[c] = take(n * sizeof(double));
    char* f[4]; for (int c = 0; c < 4; ++c) f[c] = take(n * sizeof(float));
    char* cl = take(n);
    if (w) { for (int c = 0; c < 4; ++c) w->g[c] = reinterpret_cast<double*>(g[c]);
             w->y0 = (float*)f[0]; w->x0 = (float*)f[1]; w->y1 = (float*)f[2]; w->x1 = (float*)f[3]; w->cls = (unsigned char*)cl; }
    return o;
}
size_t box_vote_workspace_bytes(int B, int64_t N) { return (B < 1 || N < 1) ? 0 : bv_ws_layout(B, N, nullptr, nullptr); }

__device__ __forceinline__ bool bv_finite(float v) { return fabsf(v) <= FLT_MAX; }          // false for NaN and inf
// a layer / prior id: finite, integral, inside [0, n)
__device__ __forceinline__ bool bv_id(float v, int n, int& out) {
    const bool ok = v >= 0.f && v < (float)n && floorf(v) == v;
    out = ok ? (int)v : 0;
    return ok;
}
// variance of coordinate c of a row: false when a part it would contribute is not finite or negative
__device__ __forceinline__ bool bv_var(const float* r, const VoteParams& p, int c, double& v) {
    bool ok = true;
    v = 0.0;
    if (p.var == BYOLO_VOTE_ALE || p.var == BYOLO_VOTE_TOTAL) { const float a = r[p.ale_col + c]; ok = ok && bv_finite(a) && a >= 0.f; v += (double)a; }
    if (p.var == BYOLO_VOTE_EPI || p.var == BYOLO_VOTE_TOTAL) { const float e = r[p.epi_col + c]; ok = ok && bv_finite(e) && e >= 0.f; v += (double)e; }
    return ok;
}
// position of a centre inside its cell: s = c * n, minus the cell's index clamped to the grid, clipped to [0, 1]
__device__ __forceinline__ double bv_frac(double c, int n) {
    const double s = c * (double)n;
    double f = floor(s);
    f = f < 0.0 ? 0.0 : (f > (double)(n - 1) ? (double)(n - 1) : f);
    const double q = s - f;
    return q < 0.0 ? 0.0 : (q > 1.0 ? 1.0 : q);
}

__global__ __launch_bounds__(256) void bv_pack_kernel(VoteParams p, BvWs w) {
    const int b = blockIdx.y;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= p.N) return;
    const size_t at = (size_t)b * p.N + i;
    const float* r = p.boxes + at * p.D;
    const float score = r[p.obj_idx];
    int cl = classify_row(r + p.cls_start, p.C, score);
    const float b0 = r[0], b1 = r[1], b2 = r[2], b3 = r[3];
    const NBox bx = make_box(b0, b1, b2, b3);
    bool ok = cl != PC_NONE && score >= p.min_score && bv_finite(b0) && bv_finite(b1) && bv_finite(b2) && bv_finite(b3);
    double gx = 1.0, gy = 1.0, gw = 1.0, gh = 1.0;
    if (ok && p.var != BYOLO_VOTE_NONE) {
        int layer = 0, prior = 0;
        ok = bv_id(r[p.geom.layer_col], p.geom.n_layers, layer);
        if (ok) ok = bv_id(r[p.geom.prior_col], p.geom.n_priors[layer], prior);
        double vx, vy, vw, vh;
        ok = bv_var(r, p, 0, vx) && ok; ok = bv_var(r, p, 1, vy) && ok; ok = bv_var(r, p, 2, vw) && ok; ok = bv_var(r, p, 3, vh) && ok;
        if (ok) {
            const int lh = p.geom.lh[layer], lw = p.geom.lw[layer];
            const double cx = ((double)bx.x0 + (double)bx.x1) * 0.5, cy = ((double)bx.y0 + (double)bx.y1) * 0.5;
            const double bw = (double)bx.x1 - (double)bx.x0, bh = (double)bx.y1 - (double)bx.y0;
            const double fx = bv_frac(cx, lw), fy = bv_frac(cy, lh);
            const double tx = fx * (1.0 - fx) / (double)lw, ty = fy * (1.0 - fy) / (double)lh;
            const double fl = (double)p.var_floor;
            gx = 1.0 / fmax(vx * (tx * tx), fl); gy = 1.0 / fmax(vy * (ty * ty), fl);
            gw = 1.0 / fmax(vw * (bw * bw), fl); gh = 1.0 / fmax(vh * (bh * bh), fl);
        }
    }
    if (!ok) cl = PC_NONE;
    w.cls[at] = (unsigned char)cl;
    w.y0[at] = bx.y0; w.x0[at] = bx.x0; w.y1[at] = bx.y1; w.x1[at] = bx.x1;
    w.g[0][at] = gx; w.g[1][at] = gy; w.g[2][at] = gw; w.g[3][at] = gh;
}

__device__ __forceinline__ NBox bv_box(float y0, float x0, float y1, float x1) {      // from corners that are already sorted
    NBox r = {y0, x0, y1, x1, 0.f};
    r.area = __fmul_rn(__fsub_rn(y1, y0), __fsub_rn(x1, x0));
    return r;
}
__device__ __forceinline__ double bv_fold(double v) {        // the 16 lanes of a kept row: butterfly, the same tree in every lane
    v += __shfl_xor(v, 1); v += __shfl_xor(v, 2); v += __shfl_xor(v, 4); v += __shfl_xor(v, 8);
    return v;
}

__global__ __launch_bounds__(256) void bv_vote_kernel(VoteParams p, BvWs w) {
    __shared__ float s_y0[BV_TILE], s_x0[BV_TILE], s_y1[BV_TILE], s_x1[BV_TILE];
    __shared__ unsigned char s_cl[BV_TILE];
    const int b = blockIdx.y, tid = threadIdx.x, kl = tid / BV_SUB, sub = tid % BV_SUB;
    const int k0 = blockIdx.x * BV_KT;
    const int nrow = p.cap - k0 < BV_KT ? p.cap - k0 : BV_KT;
    const size_t row0 = ((size_t)b * p.cap + k0) * p.D;
    if (p.rows_out != p.rows_in) {                           // not in place: every column and the padding rows come along
        for (int e = tid; e < nrow * p.D; e += 256) p.rows_out[row0 + e] = p.rows_in[row0 + e];
        __syncthreads();
    }
    int total = p.count[2 * b];
    total = total < p.cap ? total : p.cap;
    const int k = k0 + kl;
    if (k0 >= total) {                                       // padding only (uniform over the workgroup)
        if (sub == 0 && kl < nrow) p.vote_n[(size_t)b * p.cap + k] = 0;
        return;
    }
    // the kept row: its packed copy says whether it may vote at all; it must also pass the IoU test against itself
    const size_t img = (size_t)b * p.N;
    int idx = k < total ? p.kept[(size_t)b * p.cap + k] : -1;
    if (idx < 0 || (int64_t)idx >= p.N) idx = -1;
    int my_cl = PC_NONE;
    NBox me = {0.f, 0.f, 0.f, 0.f, 0.f};
    if (idx >= 0) {
        my_cl = w.cls[img + idx];
        me = bv_box(w.y0[img + idx], w.x0[img + idx], w.y1[img + idx], w.x1[img + idx]);
    }
    const bool active = my_cl != PC_NONE && iou_value(me, me) > p.iou_min;
    const double sig = (double)p.sigma_t;
    double a_x = 0.0, a_y = 0.0, a_w = 0.0, a_h = 0.0, n_x = 0.0, n_y = 0.0, n_w = 0.0, n_h = 0.0;
    int votes = 0;
    for (int64_t t0 = 0; t0 < p.N; t0 += BV_TILE) {
        for (int e = tid; e < BV_TILE; e += 256) {
            const int64_t j = t0 + e;
            const bool in = j < p.N;
            s_cl[e] = in ? w.cls[img + j] : (unsigned char)PC_NONE;
            s_y0[e] = in ? w.y0[img + j] : 0.f; s_x0[e] = in ? w.x0[img + j] : 0.f;
            s_y1[e] = in ? w.y1[img + j] : 0.f; s_x1[e] = in ? w.x1[img + j] : 0.f;
        }
        __syncthreads();
        if (active) {
            for (int e = sub; e < BV_TILE; e += BV_SUB) {
                if ((int)s_cl[e] != my_cl) continue;
                const NBox o = bv_box(s_y0[e], s_x0[e], s_y1[e], s_x1[e]);
                const float iou = iou_value(me, o);
                if (!(iou > p.iou_min)) continue;
                const size_t at = img + (size_t)(t0 + e);
                const double d = 1.0 - (double)iou;
                const double pw = exp(-(d * d) / sig);
                const double gx = pw * w.g[0][at], gy = pw * w.g[1][at], gw = pw * w.g[2][at], gh = pw * w.g[3][at];
                const double cx = ((double)o.x0 + (double)o.x1) * 0.5, cy = ((double)o.y0 + (double)o.y1) * 0.5;
                const double bw = (double)o.x1 - (double)o.x0, bh = (double)o.y1 - (double)o.y0;
                a_x += gx * cx; a_y += gy * cy; a_w += gw * bw; a_h += gh * bh;
                n_x += gx; n_y += gy; n_w += gw; n_h += gh;
                ++votes;
            }
        }
        __syncthreads();
    }
    a_x = bv_fold(a_x); a_y = bv_fold(a_y); a_w = bv_fold(a_w); a_h = bv_fold(a_h);
    n_x = bv_fold(n_x); n_y = bv_fold(n_y); n_w = bv_fold(n_w); n_h = bv_fold(n_h);
    votes += __shfl_xor(votes, 1); votes += __shfl_xor(votes, 2); votes += __shfl_xor(votes, 4); votes += __shfl_xor(votes, 8);
    if (sub != 0 || kl >= nrow) return;
    p.vote_n[(size_t)b * p.cap + k] = active ? votes : 0;
    if (!active) return;                                     // the row keeps the bits it has (in place) or was copied with
    const double cx = a_x / n_x, cy = a_y / n_y, bw = a_w / n_w, bh = a_h / n_h;
    float* ro = p.rows_out + ((size_t)b * p.cap + k) * p.D;
    ro[0] = (float)(cy - bh * 0.5); ro[1] = (float)(cx - bw * 0.5); ro[2] = (float)(cy + bh * 0.5); ro[3] = (float)(cx + bw * 0.5);
}

hipError_t launch_box_vote(const VoteParams& p, hipStream_t st) {
    if (p.B < 1 || p.B > 65535 || p.N < 1 || p.N >= (1ll << 31) || p.cap < 1 || p.C < 1 || p.C > BYOLO_MAX_CLASSES) return hipErrorInvalidValue;
    if (p.ws_bytes < bv_ws_layout(p.B, p.N, nullptr, nullptr)) return hipErrorInvalidValue;
    BvWs w;
    bv_ws_layout(p.B, p.N, reinterpret_cast<char*>(p.ws), &w);
    hipLaunchKernelGGL(bv_pack_kernel, dim3((unsigned)((p.N + 255) / 256), p.B), dim3(256), 0, st, p, w);
    hipLaunchKernelGGL(bv_vote_kernel, dim3((unsigned)((p.cap + BV_KT - 1) / BV_KT), p.B), dim3(256), 0, st, p, w);
    return hipGetLastError();
}

}  // namespace byk

// ------------------------------------------------------------------------------------------------
// C-ABI (include/byolo.h "variance voting")
// ------------------------------------------------------------------------------------------------
// The settings of a byolo_vote_cfg that do not depend on the rows; `what` names the entry point in the message.
static int32_t vote_check_settings(byolo_t* h, const byolo_vote_cfg* c, const char* what) {
    if (c->struct_bytes != (int32_t)sizeof *c) return fail(h, BYOLO_ERR_ARG, "%s: struct_bytes %d, this library's byolo_vote_cfg has %d (include/byolo.h)", what, c->struct_bytes, (int)sizeof *c);
    if (c->var < BYOLO_VOTE_NONE || c->var > BYOLO_VOTE_TOTAL) return fail(h, BYOLO_ERR_ARG, "%s: unknown var %d (BYOLO_VOTE_*)", what, c->var);
    if (!(c->sigma_t > 0.f) || !(c->sigma_t <= FLT_MAX)) return fail(h, BYOLO_ERR_ARG, "%s: sigma_t %g must be > 0 and finite", what, (double)c->sigma_t);
    if (!(c->iou_min >= 0.f)) return fail(h, BYOLO_ERR_ARG, "%s: iou_min %g must be >= 0", what, (double)c->iou_min);
    if (!(c->var_floor > 0.f) || !(c->var_floor <= FLT_MAX)) return fail(h, BYOLO_ERR_ARG, "%s: var_floor %g must be > 0 and finite", what, (double)c->var_floor);
    if (c->min_score != c->min_score) return fail(h, BYOLO_ERR_ARG, "%s: min_score is NaN", what);
    return BYOLO_OK;
}
// ... and the columns of a variance kind against a row of D floats
static int32_t vote_check_columns(byolo_t* h, int32_t var, int32_t ale_col, int32_t epi_col, int32_t D, const char* what) {
    const bool ale = var == BYOLO_VOTE_ALE || var == BYOLO_VOTE_TOTAL, epi = var == BYOLO_VOTE_EPI || var == BYOLO_VOTE_TOTAL;
    if (ale && ale_col < 0) return fail(h, BYOLO_ERR_ARG, "%s: var %d needs aleatoric variances, these rows have none (ale_col %d)", what, var, ale_col);
    if (epi && epi_col < 0) return fail(h, BYOLO_ERR_ARG, "%s: var %d needs epistemic variances, these rows have none (epi_col %d)", what, var, epi_col);
    if (ale && (int64_t)ale_col + 4 > D) return fail(h, BYOLO_ERR_ARG, "%s: ale_col %d .. +3 outside the row of %d", what, ale_col, D);
    if (epi && (int64_t)epi_col + 4 > D) return fail(h, BYOLO_ERR_ARG, "%s: epi_col %d .. +3 outside the row of %d", what, epi_col, D);
    return BYOLO_OK;
}
static int32_t vote_check_geom(byolo_t* h, const byolo_eval_loc_cfg* g, int32_t D, VoteGeom* out, const char* what) {
    if (!g) return fail(h, BYOLO_ERR_ARG, "%s: geom is NULL (only BYOLO_VOTE_NONE goes without the geometry table)", what);
    if (g->struct_bytes != (int32_t)sizeof *g) return fail(h, BYOLO_ERR_ARG, "%s: geom->struct_bytes %d, this library's byolo_eval_loc_cfg has %d", what, g->struct_bytes, (int)sizeof *g);
    if (g->layer_col < 0 || g->layer_col >= D) return fail(h, BYOLO_ERR_ARG, "%s: geom->layer_col %d outside the row", what, g->layer_col);
    if (g->prior_col < 0 || g->prior_col >= D) return fail(h, BYOLO_ERR_ARG, "%s: geom->prior_col %d outside the row", what, g->prior_col);
    if (g->n_layers < 1 || g->n_layers > BYOLO_EVAL_LOC_MAX_LAYERS) return fail(h, BYOLO_ERR_ARG, "%s: geom->n_layers %d outside 1 .. %d", what, g->n_layers, BYOLO_EVAL_LOC_MAX_LAYERS);
    memset(out, 0, sizeof *out);
    out->layer_col = g->layer_col; out->prior_col = g->prior_col; out->n_layers = g->n_layers;
    for (int l = 0; l < g->n_layers; ++l) {
        if (g->n_priors[l] < 1 || g->n_priors[l] > BYOLO_EVAL_LOC_MAX_PRIORS) return fail(h, BYOLO_ERR_ARG, "%s: geom->n_priors of layer %d outside 1 .. %d", what, l, BYOLO_EVAL_LOC_MAX_PRIORS);
        if (g->lh[l] < 1 || g->lw[l] < 1) return fail(h, BYOLO_ERR_ARG, "%s: geom: grid of layer %d is %d x %d", what, l, g->lh[l], g->lw[l]);
        out->lh[l] = g->lh[l]; out->lw[l] = g->lw[l]; out->n_priors[l] = g->n_priors[l];
    }
    return BYOLO_OK;
}

extern "C" size_t byolo_box_vote_workspace_bytes(int32_t B, int64_t N) { return box_vote_workspace_bytes(B, N); }

extern "C" int32_t byolo_box_vote(byolo_t* h, const float* d_boxes, int32_t B, int64_t N, int32_t D, int32_t obj_idx, int32_t cls_start_idx,
                                  int32_t nms_mode, const byolo_vote_cfg* cfg, const byolo_eval_loc_cfg* geom, const float* d_rows_in,
                                  const int32_t* d_kept, const int32_t* d_count, int32_t cap, float* d_rows_out, int32_t* d_vote_n,
                                  void* d_ws, size_t ws_bytes, void* stream) {
    const char* what = "byolo_box_vote";
    if (!h || !d_boxes || !cfg || !d_rows_in || !d_kept || !d_count || !d_rows_out || !d_vote_n || !d_ws) return fail(h, BYOLO_ERR_ARG, "%s: null argument", what);
    int32_t C = 0;
    int32_t rc = check_rows_shape(h, what, B, 65535, N, D, obj_idx, cls_start_idx, nms_mode, &C); if (rc) return rc;
    if (cap < 1) return fail(h, BYOLO_ERR_ARG, "%s: bad shape", what);
    rc = vote_check_settings(h, cfg, what); if (rc) return rc;
    rc = vote_check_columns(h, cfg->var, cfg->ale_col, cfg->epi_col, D, what); if (rc) return rc;
    VoteParams p; memset(&p, 0, sizeof p);
    if (cfg->var != BYOLO_VOTE_NONE) { rc = vote_check_geom(h, geom, D, &p.geom, what); if (rc) return rc; }
    if (ws_bytes < box_vote_workspace_bytes(B, N)) return fail(h, BYOLO_ERR_NOMEM, "%s: workspace %zu < byolo_box_vote_workspace_bytes(B, N) = %zu", what, ws_bytes, box_vote_workspace_bytes(B, N));
    if (reinterpret_cast<uintptr_t>(d_ws) & 7) return fail(h, BYOLO_ERR_ARG, "%s: d_ws is not 8-byte aligned", what);
    HIPCHK(h, hipSetDevice(h->device));
    p.boxes = d_boxes; p.B = B; p.N = N; p.D = D; p.obj_idx = obj_idx; p.cls_start = cls_start_idx; p.C = C;
    p.var = cfg->var; p.sigma_t = cfg->sigma_t; p.iou_min = cfg->iou_min; p.min_score = cfg->min_score; p.var_floor = cfg->var_floor;
    p.ale_col = cfg->ale_col; p.epi_col = cfg->epi_col;
    p.rows_in = d_rows_in; p.kept = d_kept; p.count = d_count; p.cap = cap; p.rows_out = d_rows_out; p.vote_n = d_vote_n;
    p.ws = d_ws; p.ws_bytes = ws_bytes;
    HIPCHK(h, launch_box_vote(p, reinterpret_cast<hipStream_t>(stream)));
    return BYOLO_OK;
}

// What byolo_forward votes with: the handle's rows (columns of the detection kind) and the grids of its detection layers.
// BYOLO_ERR_ARG when the rows cannot support the variance kind asked for.
int32_t byolo_vote_from_handle(byolo_t* h, VoteParams* p, const char* what) {
    const byolo_vote_cfg& c = h->vote_cfg;
    memset(p, 0, sizeof *p);
    int kind = -1, n = 0;
    for (const Layer& l : h->layers) {
        if (l.op != OP_DETECTION) continue;
        kind = l.det_kind;
        if (n < BYOLO_EVAL_LOC_MAX_LAYERS) { p->geom.lh[n] = l.H; p->geom.lw[n] = l.W; p->geom.n_priors[n] = 3; }
        ++n;
    }
    if (kind < 0) return fail(h, BYOLO_ERR_STATE, "%s: box voting needs a detection layer", what);
    const int32_t ale_col = kind == BYOLO_DET_ALEATORIC ? 4 : kind == BYOLO_DET_EPISTEMIC ? 8 : -1, epi_col = kind == BYOLO_DET_EPISTEMIC ? 4 : -1;
    int32_t rc = vote_check_columns(h, c.var, ale_col, epi_col, h->row_len, what); if (rc) return rc;
    if (c.var != BYOLO_VOTE_NONE) {
        if (n > BYOLO_EVAL_LOC_MAX_LAYERS) return fail(h, BYOLO_ERR_ARG, "%s: box voting takes up to %d detection layers, the graph has %d", what, BYOLO_EVAL_LOC_MAX_LAYERS, n);
        p->geom.n_layers = n;
        p->geom.layer_col = h->row_len - 2; p->geom.prior_col = h->row_len - 1;      // the decode's last two columns (12 + C, 13 + C / 19 + C, 20 + C)
    }
    p->var = c.var; p->sigma_t = c.sigma_t; p->iou_min = c.iou_min; p->min_score = c.min_score; p->var_floor = c.var_floor;
    p->ale_col = ale_col; p->epi_col = epi_col;
    p->D = h->row_len; p->obj_idx = h->obj_idx; p->cls_start = h->cls_start; p->N = h->n_boxes;
    p->C = nms_classes(h->cfg.nms_mode, h->cfg.cls_cnt);
    return BYOLO_OK;
}

extern "C" int32_t byolo_set_box_vote(byolo_t* h, const byolo_vote_cfg* cfg) {
    if (!h) return fail(nullptr, BYOLO_ERR_ARG, "byolo_set_box_vote: null handle");
    if (cfg) {
        int32_t rc = vote_check_settings(h, cfg, "byolo_set_box_vote"); if (rc) return rc;
        if (h->n_det) {                                      // a graph that already has its detection layers: refuse now what byolo_forward would
            const byolo_vote_cfg keep = h->vote_cfg;
            VoteParams p;
            h->vote_cfg = *cfg;
            rc = byolo_vote_from_handle(h, &p, "byolo_set_box_vote");
            h->vote_cfg = keep;
            if (rc) return rc;
        }
        h->vote_cfg = *cfg;
    }
    h->vote_on = cfg != nullptr;
    side_out_forget(&h->out_vote_n);
    // the stage's workspace is part of the plan, and a captured forward holds the launches of the old setting
    invalidate_plan(h);
    return BYOLO_OK;
}

extern "C" int32_t byolo_box_vote_counts(byolo_t* h, int32_t* d_vote_n, int32_t B, int32_t cap, void* stream) {
    if (!h || !d_vote_n) return fail(h, BYOLO_ERR_ARG, "byolo_box_vote_counts: null argument");
    if (!h->out_vote_n.ptr) return fail(h, BYOLO_ERR_STATE, "byolo_box_vote_counts: no byolo_forward with box voting (byolo_set_box_vote) and d_rows has run on this handle");
    return side_out_copy(h, &h->out_vote_n, d_vote_n, B, cap, "byolo_box_vote_counts", stream);
}
