// nms_box.h -- the box and the IoU that the NMS (tail_kernels.hip) and the evaluation matcher (eval_kernels.hip) share.
// IoU is evaluated operation-for-operation as TensorFlow's IOU() in float32 with single rounding (__f*_rn: no FMA
// contraction), std::min/std::max NaN semantics.
#pragma once
#include <hip/hip_runtime.h>

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

}  // namespace byk
