// nms_box.h -- the box and the IoU that the NMS (tail_kernels.hip), the evaluation matcher (eval_kernels.hip) and variance
// voting (box_vote.hip) share, and the score key / class of a row that the NMS and the voting agree on.
// IoU is evaluated operation-for-operation as TensorFlow's IOU() in float32 with single rounding (__f*_rn: no FMA
// contraction), std::min/std::max NaN semantics.
#pragma once
#include <hip/hip_runtime.h>

#include <cfloat>

namespace byk {

struct NBox { float y0, x0, y1, x1, area; };

__device__ __forceinline__ float smin_(float a, float b) { return (b < a) ? b : a; }
__device__ __forceinline__ float smax_(float a, float b) { return (a < b) ? b : a; }

__device__ __forceinline__ NBox make_box(float b0, float b1, float b2, float b3) {
    NBox r;
    r.y0 = smin_(b0, b2); r.x0 = smin_(b1, b3);
    r.y1 = smax_(b0, b2); r.x1 = smax_(b1, b3);
    r.area = __fmul_rn(__fsub_rn(r.y1, r.y0), __fsub_rn(r.x1, r.x0));
    return r;
}
// IoU of two boxes of positive area
__device__ __forceinline__ float iou_of(const NBox& i, const NBox& j) {
    const float iy0 = smax_(i.y0, j.y0), ix0 = smax_(i.x0, j.x0);
    const float iy1 = smin_(i.y1, j.y1), ix1 = smin_(i.x1, j.x1);
    const float inter = __fmul_rn(smax_(__fsub_rn(iy1, iy0), 0.f), smax_(__fsub_rn(ix1, ix0), 0.f));
    return __fdiv_rn(inter, __fsub_rn(__fadd_rn(i.area, j.area), inter));
}
__device__ __forceinline__ bool iou_gt(const NBox& i, const NBox& j, float thr) {
    if (i.area <= 0.f || j.area <= 0.f) return false;        // IoU = 0
    return iou_of(i, j) > thr;
}
// the value instead of the comparison: 0 when either area is <= 0
__device__ __forceinline__ float iou_value(const NBox& i, const NBox& j) {
    if (i.area <= 0.f || j.area <= 0.f) return 0.f;
    return iou_of(i, j);
}
// iou_value with one rounding per operation whatever the file's contraction mode: for callers that hand the VALUE on -- the
// soft-NMS multiplies scores by a weight of it -- and are compared bit for bit with numpy.  Plain operators under the pragma: the
// __f*_rn intrinsics above are inlined header functions whose operators keep the contraction mode of the file, and the product
// `inter` then fuses into the subtraction behind it.  (A float32 quotient is correctly rounded in every mode of this build.)
__device__ __forceinline__ float iou_value_rn(const NBox& i, const NBox& j) {
#pragma clang fp contract(off)
    if (i.area <= 0.f || j.area <= 0.f) return 0.f;
    const float iy0 = smax_(i.y0, j.y0), ix0 = smax_(i.x0, j.x0);
    const float iy1 = smin_(i.y1, j.y1), ix1 = smin_(i.x1, j.x1);
    const float inter = smax_(iy1 - iy0, 0.f) * smax_(ix1 - ix0, 0.f);
    const float uni = (i.area + j.area) - inter;
    return inter / uni;
}

// ---- score and class of a row, as the NMS pipeline (tail_kernels.hip pc_*) and the vote stage (box_vote.hip) decide them ----
__device__ __forceinline__ unsigned int score_key(float f) {
    // ascending key == descending score; NaN and scores <= -FLT_MAX are not candidates
    // (TF: `score > std::numeric_limits<float>::lowest()`), they sort last.  Equal scores are equal keys: -0.0 == +0.0,
    // so either zero takes the key of +0.0 and the row index alone orders them (a select: `f + 0.f` may be folded away).
    if (!(f > -FLT_MAX)) return 0xFFFFFFFFu;
    unsigned int u = (f == 0.f) ? 0u : __float_as_uint(f);
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ~u;
}

static constexpr int PC_NONE = 255;                          // class byte of a row that belongs to no class

// The class of one row from its C class scores `t` (global memory or LDS) and its score: class c iff cls[c] > cls[k] for every
// k != c -- a maximum attained twice or any NaN leaves no such c; a score that is no NMS candidate leaves none either.
// One class: every candidate is a member and `t` is not read (the rows of BYOLO_NMS_AGNOSTIC need not have class columns).
__device__ __forceinline__ int classify_row(const float* t, int C, float score) {
    if (score_key(score) == 0xFFFFFFFFu) return PC_NONE;
    if (C == 1) return 0;
    float best = t[0];
    int arg = 0;
    bool uniq = true, nan = best != best;
    for (int c = 1; c < C; ++c) {
        const float v = t[c];
        nan |= v != v;
        if (v > best) { best = v; arg = c; uniq = true; }
        else if (v == best) uniq = false;
    }
    return (uniq && !nan) ? arg : PC_NONE;
}

}  // namespace byk
