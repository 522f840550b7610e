// tta.hip -- test-time augmentation (include/byolo.h "test-time augmentation"; INTEGRATION.md has the definitions in full,
// tests/_tta_ref.py restates them in numpy): the same frame is run mirrored and / or at a second size, every view's pre-NMS rows
// go into ONE candidate set per image, and the NMS, the voting and the score stage work on that union.
//
//   tta_view    float32 frames [B, sh, sw, 3] -> the view's image [B, oh, ow, 3]: steps 2 and 3 of augment.hip (TF1's legacy bilinear
//               resize, src = dst * in / out without a half-pixel offset, then the left-right flip) on float inputs, operation for
//               operation -- the file is compiled with contraction off and correctly rounded division (csrc/build.py FILE_FLAGS),
//               so the output is the bytes byolo_augment_batch writes for the uint8 frame whose * (1 / 255) is the input.
//               One lane per output pixel; the same size is a mirrored copy.
//   tta_merge   one launch per view, one lane per float: the view's rows [B, Nv, D] into the union [B, Nu, D] at row `off`.
//               A mirrored view: column 1 = 1 - column 3, column 3 = 1 - column 1 (one float32 subtraction; a NaN keeps its bits).
//               The layer id of a view at the g-th size gains 3 g (finite ids only, g > 0 only).  Everything else keeps its bits.
//   tta_pack    once per batch, one lane per union row: class byte (classify_row of nms_box.h -- the NMS's own decision), sorted
//               corners, and the score where the row may be a witness at all (score >= min_score, four finite box values), NaN
//               where it may not.  Index-aligned SoA, as bv_pack of box_vote.hip.
//   tta_support one wave per kept row.  Per view (a compile-time unrolled loop: no private segment) the 64 lanes stride over the
//               view's rows, each keeps its best (score, lowest index); a butterfly over the total order (score descending, index
//               ascending) leaves the view's witness in every lane, and lane v keeps view v's.  Lanes 0 .. V-1 then load their
//               witness; the float64 sums run over `__shfl(x, v)` in view order in every lane alike, lane 0 writes.
//
// The argmax over a total order makes the lane assignment irrelevant; nothing depends on which workgroup runs first or on the
// image's position in the batch.  Every [B, cap] slot is written by the kernel itself (zeros in the padding): nothing to clear.
#include "byolo_internal.h"
#include "nms_box.h"

#pragma clang fp contract(off)

namespace byk {

// ---- view -------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void tta_view_kernel(const float* __restrict__ src, int sh, int sw, int flip, int oh, int ow, float* __restrict__ out) {
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= (int64_t)oh * ow) return;
    const int i = (int)(q / ow), j = (int)(q % ow);
    const float* img = src + (int64_t)blockIdx.y * sh * sw * 3;
    float* d = out + ((int64_t)blockIdx.y * oh * ow + q) * 3;
    const int jj = flip ? ow - 1 - j : j;
    if (sh == oh && sw == ow) {
        const float* s = img + ((int64_t)i * sw + jj) * 3;
        d[0] = s[0]; d[1] = s[1]; d[2] = s[2];
        return;
    }
    const float hs = (float)sh / (float)oh, ws = (float)sw / (float)ow;
    const float iny = (float)i * hs, fy = floorf(iny);
    const float inx = (float)jj * ws, fx = floorf(inx);
    const int ylo = min(max((int)fy, 0), sh - 1), yhi = min((int)ceilf(iny), sh - 1);
    const int xlo = min(max((int)fx, 0), sw - 1), xhi = min((int)ceilf(inx), sw - 1);
    const float ly = iny - fy, lx = inx - fx;
    const float* rt = img + (int64_t)ylo * sw * 3;
    const float* rb = img + (int64_t)yhi * sw * 3;
    for (int c = 0; c < 3; ++c) {
        const float tl = rt[xlo * 3 + c], tr = rt[xhi * 3 + c];
        const float bl = rb[xlo * 3 + c], br = rb[xhi * 3 + c];
        const float top = tl + (tr - tl) * lx;
        const float bottom = bl + (br - bl) * lx;
        d[c] = top + (bottom - top) * ly;
    }
}

// ---- merge ------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool tta_finite(float v) { return fabsf(v) <= FLT_MAX; }          // false for NaN and inf

__global__ __launch_bounds__(256) void tta_merge_kernel(const float* __restrict__ src, int64_t Nv, int D, int flip, int layer_col, float id_add,
                                                        float* __restrict__ dst, int64_t Nu, int64_t off) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= Nv * D) return;
    const int64_t i = e / D;
    const int c = (int)(e - i * D);
    const float* r = src + ((int64_t)blockIdx.y * Nv + i) * D;
    float v = r[c];
    if (flip && (c == 1 || c == 3)) {
        const float o = r[4 - c];
        const unsigned int ob = __float_as_uint(o);          // the select runs on the bit patterns: a NaN keeps its payload
        v = __uint_as_float((ob & 0x7FFFFFFFu) > 0x7F800000u ? ob : __float_as_uint(1.0f - o));
    } else if (c == layer_col && id_add != 0.f && tta_finite(v)) {
        v = v + id_add;
    }
    dst[((int64_t)blockIdx.y * Nu + off + i) * D + c] = v;
}

// ---- support ----------------------------------------------------------------------------------------------------------------------
struct TtaWs {
    float *y0, *x0, *y1, *x1, *sc;                           // [B][Nu] corners as make_box sorts them; the score of a possible witness, NaN otherwise
    unsigned char* cls;                                      // [B][Nu] classify_row of the row
};
static size_t tta_ws_layout(int B, int64_t N, char* base, TtaWs* w) {
    size_t o = 0;
    auto take = [&](size_t bytes) { char* p = base ? base + o : nullptr; o += (bytes + 255) / 256 * 256; return p; };
    const size_t n = (size_t)B * (size_t)N;
    char* f[5]; for (int c = 0; c < 5; ++c) f[c] = take(n * sizeof(float));
    char* cl = take(n);
    if (w) { w->y0 = (float*)f[0]; w->x0 = (float*)f[1]; w->y1 = (float*)f[2]; w->x1 = (float*)f[3]; w->sc = (float*)f[4]; w->cls = (unsigned char*)cl; }
    return o;
}

struct TtaSupportParams {
    const float* boxes; int B; int64_t N; int D, obj_idx, cls_start, C;
    int V; float iou_min, min_score; int off[9];
    const int32_t* kept; const int32_t* count; int cap;
    int32_t *view_n, *view_bits; float *view_score, *view_var;
};

__global__ __launch_bounds__(256) void tta_pack_kernel(TtaSupportParams p, TtaWs w) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= p.N) return;
    const size_t at = (size_t)blockIdx.y * p.N + i;
    const float* r = p.boxes + at * p.D;
    const float score = r[p.obj_idx];
    const float b0 = r[0], b1 = r[1], b2 = r[2], b3 = r[3];
    const NBox bx = make_box(b0, b1, b2, b3);
    const bool ok = score >= p.min_score && tta_finite(b0) && tta_finite(b1) && tta_finite(b2) && tta_finite(b3);
    w.cls[at] = (unsigned char)classify_row(r + p.cls_start, p.C, score);
    w.y0[at] = bx.y0; w.x0[at] = bx.x0; w.y1[at] = bx.y1; w.x1[at] = bx.x1;
    w.sc[at] = ok ? score : __uint_as_float(0x7FC00000u);
}

__device__ __forceinline__ NBox tta_box(float y0, float x0, float y1, float x1) {      // from corners that are already sorted
    NBox r = {y0, x0, y1, x1, 0.f};
    r.area = __fmul_rn(__fsub_rn(y1, y0), __fsub_rn(x1, x0));
    return r;
}
// (s, i) before (bs, bi) in the total order: score descending, index ascending; i < 0 is no candidate
__device__ __forceinline__ bool tta_better(float s, int i, float bs, int bi) {
    if (i < 0) return false;
    if (bi < 0) return true;
    return s > bs || (s == bs && i < bi);
}

__global__ __launch_bounds__(256) void tta_support_kernel(TtaSupportParams p, TtaWs w) {
    const int b = blockIdx.y, lane = threadIdx.x & 63;
    const int k = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (k >= p.cap) return;                                  // uniform over the wave
    const size_t slot = (size_t)b * p.cap + k;
    int total = p.count[2 * b];
    total = total < p.cap ? total : p.cap;
    const size_t img = (size_t)b * p.N;
    int idx = k < total ? p.kept[slot] : -1;
    if (idx < 0 || (int64_t)idx >= p.N) idx = -1;
    int my_cl = PC_NONE;
    NBox me = {0.f, 0.f, 0.f, 0.f, 0.f};
    if (idx >= 0) {
        my_cl = w.cls[img + idx];
        me = tta_box(w.y0[img + idx], w.x0[img + idx], w.y1[img + idx], w.x1[img + idx]);
    }
    int wit = -1;                                            // lane v: the witness of view v
    if (my_cl != PC_NONE) {                                  // uniform over the wave
#pragma unroll
        for (int v = 0; v < 8; ++v) {
            if (v >= p.V) break;
            float bs = 0.f;
            int bi = -1;
            for (int i = p.off[v] + lane; i < p.off[v + 1]; i += 64) {
                if ((int)w.cls[img + i] != my_cl) continue;
                const float s = w.sc[img + i];
                if (s != s) continue;
                const NBox o = tta_box(w.y0[img + i], w.x0[img + i], w.y1[img + i], w.x1[img + i]);
                if (!(iou_value(me, o) > p.iou_min)) continue;
                if (tta_better(s, i, bs, bi)) { bs = s; bi = i; }
            }
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) {
                const float os = __shfl_xor(bs, m);
                const int oi = __shfl_xor(bi, m);
                if (tta_better(os, oi, bs, bi)) { bs = os; bi = oi; }
            }
            if (lane == v) wit = bi;
        }
    }
    const bool has = wit >= 0;
    double sc = 0.0, cx = 0.0, cy = 0.0, bw = 0.0, bh = 0.0;
    if (has) {
        const float y0 = w.y0[img + wit], x0 = w.x0[img + wit], y1 = w.y1[img + wit], x1 = w.x1[img + wit];
        sc = (double)w.sc[img + wit];
        cx = ((double)x0 + (double)x1) * 0.5; cy = ((double)y0 + (double)y1) * 0.5;
        bw = (double)x1 - (double)x0; bh = (double)y1 - (double)y0;
    }
    const unsigned long long mask = __ballot(has);
    const int bits = (int)(mask & 0xFFull), n = __popcll(mask & 0xFFull);
    double s_sc = 0.0, s_x = 0.0, s_y = 0.0, s_w = 0.0, s_h = 0.0;
    for (int v = 0; v < p.V; ++v) {                          // view order, the same sums in every lane
        const double a = __shfl(sc, v), x = __shfl(cx, v), y = __shfl(cy, v), ww = __shfl(bw, v), hh = __shfl(bh, v);
        if ((bits >> v) & 1) { s_sc = s_sc + a; s_x = s_x + x; s_y = s_y + y; s_w = s_w + ww; s_h = s_h + hh; }
    }
    double v_x = 0.0, v_y = 0.0, v_w = 0.0, v_h = 0.0;
    if (n > 1) {
        const double dn = (double)n;
        const double m_x = s_x / dn, m_y = s_y / dn, m_w = s_w / dn, m_h = s_h / dn;
        for (int v = 0; v < p.V; ++v) {
            const double x = __shfl(cx, v) - m_x, y = __shfl(cy, v) - m_y, ww = __shfl(bw, v) - m_w, hh = __shfl(bh, v) - m_h;
            if ((bits >> v) & 1) { v_x = v_x + x * x; v_y = v_y + y * y; v_w = v_w + ww * ww; v_h = v_h + hh * hh; }
        }
        v_x = v_x / dn; v_y = v_y / dn; v_w = v_w / dn; v_h = v_h / dn;
    }
    if (lane != 0) return;
    p.view_n[slot] = n;
    p.view_bits[slot] = bits;
    p.view_score[slot] = (float)(s_sc / (double)p.V);
    float* vv = p.view_var + slot * 4;
    vv[0] = (float)v_x; vv[1] = (float)v_y; vv[2] = (float)v_w; vv[3] = (float)v_h;
}

}  // namespace byk

// ------------------------------------------------------------------------------------------------
// C-ABI (include/byolo.h "test-time augmentation")
// ------------------------------------------------------------------------------------------------
using namespace byk;

extern "C" int32_t byolo_tta_view_f32(const float* d_in, int32_t B, int32_t src_h, int32_t src_w, int32_t flip, int32_t out_h, int32_t out_w,
                                      float* d_out, void* stream) {
    const char* what = "byolo_tta_view_f32";
    if (B < 1) return BYOLO_OK;
    if (!d_in || !d_out) return fail(nullptr, BYOLO_ERR_ARG, "%s: d_in / d_out is NULL", what);
    if ((reinterpret_cast<uintptr_t>(d_in) | reinterpret_cast<uintptr_t>(d_out)) & 3) return fail(nullptr, BYOLO_ERR_ARG, "%s: d_in / d_out must be 4-byte aligned", what);
    if (B > 65535) return fail(nullptr, BYOLO_ERR_ARG, "%s: B %d beyond 65535", what, B);
    if (src_h < 1 || src_w < 1 || out_h < 1 || out_w < 1 || (int64_t)src_h * src_w * 3 >= (1ll << 31) || (int64_t)out_h * out_w * 3 >= (1ll << 31))
        return fail(nullptr, BYOLO_ERR_ARG, "%s: sizes %d x %d -> %d x %d out of range", what, src_h, src_w, out_h, out_w);
    if (flip != 0 && flip != 1) return fail(nullptr, BYOLO_ERR_ARG, "%s: flip must be 0 or 1", what);
    if (ranges_overlap(d_in, (size_t)B * src_h * src_w * 12, d_out, (size_t)B * out_h * out_w * 12)) return fail(nullptr, BYOLO_ERR_ARG, "%s: d_out overlaps d_in", what);
    const int64_t px = (int64_t)out_h * out_w;
    hipLaunchKernelGGL(tta_view_kernel, dim3((unsigned)((px + 255) / 256), B), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), d_in, src_h, src_w, flip,
                       out_h, out_w, d_out);
    HIPCHK(nullptr, hipGetLastError());
    return BYOLO_OK;
}

extern "C" int32_t byolo_tta_merge(const float* d_rows, int32_t B, int64_t Nv, int32_t D, int32_t kind, int32_t layer_col, int32_t flip, int32_t size_idx,
                                   float* d_union, int64_t Nu, int64_t row_off, void* stream) {
    const char* what = "byolo_tta_merge";
    if (kind < BYOLO_DET_STANDARD || kind > BYOLO_DET_EPISTEMIC) return fail(nullptr, BYOLO_ERR_ARG, "%s: unknown kind %d (BYOLO_DET_*)", what, kind);
    const int base = kind == BYOLO_DET_STANDARD ? 5 : kind == BYOLO_DET_ALEATORIC ? 14 : 21;
    if (D < base + 1 || D > base + 128) return fail(nullptr, BYOLO_ERR_ARG, "%s: D %d: rows of kind %d have %d + C columns, C in 1 .. 128", what, D, kind, base);
    const int want_col = kind == BYOLO_DET_STANDARD ? -1 : D - 2;
    if (layer_col != want_col) return fail(nullptr, BYOLO_ERR_ARG, "%s: layer_col %d: rows of kind %d and %d columns take %d", what, layer_col, kind, D, want_col);
    if (flip != 0 && flip != 1) return fail(nullptr, BYOLO_ERR_ARG, "%s: flip must be 0 or 1", what);
    if (size_idx < 0 || 3 * (size_idx + 1) > BYOLO_EVAL_LOC_MAX_LAYERS) return fail(nullptr, BYOLO_ERR_ARG, "%s: size_idx %d outside 0 .. %d", what, size_idx, BYOLO_EVAL_LOC_MAX_LAYERS / 3 - 1);
    if (B > 65535) return fail(nullptr, BYOLO_ERR_ARG, "%s: B %d beyond 65535", what, B);
    if (Nu < 0 || Nu >= (1ll << 31)) return fail(nullptr, BYOLO_ERR_ARG, "%s: Nu %lld out of range", what, (long long)Nu);
    if (Nv >= 1 && (row_off < 0 || row_off > Nu || Nv > Nu - row_off)) return fail(nullptr, BYOLO_ERR_ARG, "%s: row_off %lld + Nv %lld beyond Nu %lld", what, (long long)row_off, (long long)Nv, (long long)Nu);
    if (B < 1 || Nv < 1) return BYOLO_OK;
    if (!d_rows) return fail(nullptr, BYOLO_ERR_ARG, "%s: d_rows is NULL", what);
    if (!d_union) return fail(nullptr, BYOLO_ERR_ARG, "%s: d_union is NULL", what);
    if (reinterpret_cast<uintptr_t>(d_rows) & 3) return fail(nullptr, BYOLO_ERR_ARG, "%s: d_rows must be 4-byte aligned", what);
    if (reinterpret_cast<uintptr_t>(d_union) & 3) return fail(nullptr, BYOLO_ERR_ARG, "%s: d_union must be 4-byte aligned", what);
    if (ranges_overlap(d_rows, (size_t)B * Nv * D * 4, d_union, (size_t)B * Nu * D * 4)) return fail(nullptr, BYOLO_ERR_ARG, "%s: d_union overlaps d_rows", what);
    const int64_t n = Nv * D;
    hipLaunchKernelGGL(tta_merge_kernel, dim3((unsigned)((n + 255) / 256), B), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), d_rows, Nv, D, flip, layer_col,
                       (float)(3 * size_idx), d_union, Nu, row_off);
    HIPCHK(nullptr, hipGetLastError());
    return BYOLO_OK;
}

extern "C" size_t byolo_tta_support_workspace_bytes(int32_t B, int64_t Nu) { return (B < 1 || Nu < 1) ? 0 : tta_ws_layout(B, Nu, nullptr, nullptr); }

extern "C" int32_t byolo_tta_support(byolo_t* h, const float* d_union, int32_t B, int64_t Nu, int32_t D, int32_t obj_idx, int32_t cls_start_idx,
                                     int32_t nms_mode, const byolo_tta_support_cfg* cfg, const int32_t* d_kept, const int32_t* d_count, int32_t cap,
                                     int32_t* d_view_n, int32_t* d_view_bits, float* d_view_score, float* d_view_var, void* d_ws, size_t ws_bytes,
                                     void* stream) {
    const char* what = "byolo_tta_support";
    if (!h || !d_union || !cfg || !d_kept || !d_count || !d_view_n || !d_view_bits || !d_view_score || !d_view_var || !d_ws) return fail(h, BYOLO_ERR_ARG, "%s: null argument", what);
    int32_t C = 0;
    int32_t rc = check_rows_shape(h, what, B, 65535, Nu, D, obj_idx, cls_start_idx, nms_mode, &C); if (rc) return rc;
    if (cap < 1) return fail(h, BYOLO_ERR_ARG, "%s: bad shape (cap %d)", what, cap);
    if (cfg->struct_bytes != (int32_t)sizeof *cfg) return fail(h, BYOLO_ERR_ARG, "%s: struct_bytes %d, this library's byolo_tta_support_cfg has %d (include/byolo.h)", what, cfg->struct_bytes, (int)sizeof *cfg);
    if (cfg->n_views < 1 || cfg->n_views > BYOLO_TTA_MAX_VIEWS) return fail(h, BYOLO_ERR_ARG, "%s: n_views %d outside 1 .. %d", what, cfg->n_views, BYOLO_TTA_MAX_VIEWS);
    if (!(cfg->iou_min >= 0.f)) return fail(h, BYOLO_ERR_ARG, "%s: iou_min %g must be >= 0", what, (double)cfg->iou_min);
    if (cfg->min_score != cfg->min_score) return fail(h, BYOLO_ERR_ARG, "%s: min_score is NaN", what);
    if (cfg->view_off[0] != 0) return fail(h, BYOLO_ERR_ARG, "%s: view_off[0] is %d, the first view starts at row 0", what, cfg->view_off[0]);
    for (int v = 0; v < cfg->n_views; ++v)
        if (cfg->view_off[v + 1] < cfg->view_off[v] || (int64_t)cfg->view_off[v + 1] > Nu)
            return fail(h, BYOLO_ERR_ARG, "%s: view_off[%d] = %d: the offsets must ascend and stay within Nu = %lld", what, v + 1, cfg->view_off[v + 1], (long long)Nu);
    if (ws_bytes < byolo_tta_support_workspace_bytes(B, Nu)) return fail(h, BYOLO_ERR_NOMEM, "%s: workspace %zu < byolo_tta_support_workspace_bytes(B, Nu) = %zu", what, ws_bytes, byolo_tta_support_workspace_bytes(B, Nu));
    if (reinterpret_cast<uintptr_t>(d_ws) & 3) return fail(h, BYOLO_ERR_ARG, "%s: d_ws is not 4-byte aligned", what);
    if ((reinterpret_cast<uintptr_t>(d_union) | reinterpret_cast<uintptr_t>(d_kept) | reinterpret_cast<uintptr_t>(d_count) | reinterpret_cast<uintptr_t>(d_view_n) |
         reinterpret_cast<uintptr_t>(d_view_bits) | reinterpret_cast<uintptr_t>(d_view_score) | reinterpret_cast<uintptr_t>(d_view_var)) & 3)
        return fail(h, BYOLO_ERR_ARG, "%s: a device pointer is not 4-byte aligned", what);
    HIPCHK(h, hipSetDevice(h->device));
    TtaSupportParams p; memset(&p, 0, sizeof p);
    p.boxes = d_union; p.B = B; p.N = Nu; p.D = D; p.obj_idx = obj_idx; p.cls_start = cls_start_idx; p.C = C;
    p.V = cfg->n_views; p.iou_min = cfg->iou_min; p.min_score = cfg->min_score;
    for (int v = 0; v <= cfg->n_views; ++v) p.off[v] = cfg->view_off[v];
    p.kept = d_kept; p.count = d_count; p.cap = cap;
    p.view_n = d_view_n; p.view_bits = d_view_bits; p.view_score = d_view_score; p.view_var = d_view_var;
    TtaWs w;
    tta_ws_layout(B, Nu, reinterpret_cast<char*>(d_ws), &w);
    const hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(tta_pack_kernel, dim3((unsigned)((Nu + 255) / 256), B), dim3(256), 0, st, p, w);
    hipLaunchKernelGGL(tta_support_kernel, dim3((unsigned)((cap + 3) / 4), B), dim3(256), 0, st, p, w);
    HIPCHK(h, hipGetLastError());
    return BYOLO_OK;
}
