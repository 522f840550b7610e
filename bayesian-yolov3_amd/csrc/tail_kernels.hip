// tail_kernels.hip -- anchor decode (K6), MC-sample aggregation + decode (K7), score order (K8) and
// greedy NMS + gather (K9) of SURVEY.md section 2.1, as wavefront-level gfx950 kernels.
//
//   decode_std / decode_ale : lib_yolo/layers.py:11-84 (split) + :191-346 (decode) + :349-358 (entropies)
//   decode_epi              : lib_yolo/layers.py:361-411 (T-reduction) + :414-502 (decode)
//   all three write rows straight at their concat_bbox position (inference_epistemic.py:173-184,
//   inference_aleatoric.py:181-192): n = base(layer) + prior*lh*lw + row*lw + col
//   pc_* (one NMS per class): tf.image.non_max_suppression(boxes[:, :4], boxes[:, obj_idx], 1000) + tf.gather
//                             (inference_epistemic.py:99-128 incl. the commented 2-class variant), for 1, 2 or cls_cnt classes
// HBM-bound / dependency-bound byte work: no MFMA here.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <float.h>
#include "byolo_kernels.h"
#include "nms_box.h"

namespace byk {

// ------------------------------------------------------------------------------------------------
// element-wise maths (IEEE semantics kept: 0*log(0) = NaN exactly like the reference, App. D.2)
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ float sigmoidf_(float x) { return 1.0f / (1.0f + expf(-x)); }
__device__ __forceinline__ float logistic_entropy_(float s) {          // layers.py:349-353
    const float no_obj = (1.0f - s) * logf(1.0f - s);
    const float obj = s * logf(s);
    return -(no_obj + obj);
}
// Class counts: the kernels are compiled for a capacity CM of class slots held in registers.  EXACT: the class count
// IS CM (the common counts: every loop bound is a constant); otherwise the runtime count C <= CM masks the slots.
template <int CM, bool EXACT>
__device__ __forceinline__ void softmax_(const float* x, float* p, int C) {   // tf.nn.softmax (max-subtracted)
    float mx = x[0];
#pragma unroll
    for (int c = 1; c < CM; ++c) if (EXACT || c < C) mx = fmaxf(mx, x[c]);
    float sum = 0.f;
#pragma unroll
    for (int c = 0; c < CM; ++c) if (EXACT || c < C) { p[c] = expf(x[c] - mx); sum += p[c]; }
#pragma unroll
    for (int c = 0; c < CM; ++c) if (EXACT || c < C) p[c] = p[c] / sum;
}
template <int CM, bool EXACT>
__device__ __forceinline__ float softmax_entropy_(const float* p, int C) {    // layers.py:356-358
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < CM; ++c) if (EXACT || c < C) s += p[c] * logf(p[c]);
    return -s;
}
__device__ __forceinline__ void corners_(float tx, float ty, float tw, float th, int col, int row, int lw, int lh,
                                         float pw, float ph, float* o /*y0,x0,y1,x1*/) {
    // layers.py:237-249 / :316-328 / :471-483
    const float x = ((float)col + sigmoidf_(tx)) / (float)lw;
    const float y = ((float)row + sigmoidf_(ty)) / (float)lh;
    const float w = expf(tw) * pw, h = expf(th) * ph;
    const float w2 = w / 2, h2 = h / 2;
    o[0] = y - h2; o[1] = x - w2; o[2] = y + h2; o[3] = x + w2;
}

// thread <-> (image b, cell, prior p), prior fastest: a wave reads 64 * blk contiguous floats.
template <int CM, bool EXACT>
__global__ __launch_bounds__(256) void decode_std_kernel(const DecodeParams p) {
    const int C = EXACT ? CM : p.C;
    const int BLK = 5 + C, D = 5 + C;
    const int LDC = p.ld ? p.ld : 3 * BLK;
    const int cells = p.lh * p.lw;
    const int64_t total = (int64_t)p.B * cells * 3;
    for (int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; gid < total;
         gid += (int64_t)gridDim.x * blockDim.x) {
        const int pr = (int)(gid % 3);
        const int64_t bc = gid / 3;
        const int cell = (int)(bc % cells), b = (int)(bc / cells);
        const float* d = p.raw + (size_t)bc * LDC + pr * BLK;
        float v[5 + CM];
        float chk = 0.f;                                        // stays 0 unless a raw value is inf / NaN (x * 0 is NaN then)
#pragma unroll
        for (int i = 0; i < 5 + CM; ++i) if (EXACT || i < BLK) { v[i] = d[i]; chk = fmaf(v[i], 0.f, chk); }
        if (chk != 0.f && p.status) atomicOr(p.status, 2u);
        float out[5 + CM];
        corners_(v[0], v[1], v[2], v[3], cell % p.lw, cell / p.lw, p.lw, p.lh, p.pw[pr], p.ph[pr], out);
        out[4] = sigmoidf_(v[4]);
        softmax_<CM, EXACT>(v + 5, out + 5, C);
        float* o = p.boxes + ((size_t)b * p.n_total + p.box_base + (size_t)pr * cells + cell) * D;
#pragma unroll
        for (int i = 0; i < 5 + CM; ++i) if (EXACT || i < D) o[i] = out[i];
    }
}

template <int CM, bool EXACT>
__global__ __launch_bounds__(256) void decode_ale_kernel(const DecodeParams p) {
    const int C = EXACT ? CM : p.C;
    const int BLK = 2 * (5 + C), D = 14 + C;
    const int LDC = p.ld ? p.ld : 3 * BLK;
    const int cells = p.lh * p.lw;
    const int64_t total = (int64_t)p.B * cells * 3;
    for (int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; gid < total;
         gid += (int64_t)gridDim.x * blockDim.x) {
        const int pr = (int)(gid % 3);
        const int64_t bc = gid / 3;
        const int cell = (int)(bc % cells), b = (int)(bc / cells);
        const float* d = p.raw + (size_t)bc * LDC + pr * BLK;
        // [x,y,w,h, logvar x4, obj, log_obj_std, cls xC, log_cls_std xC]   (layers.py:41-84); the stds are not decoded
        float v[10 + CM];
        float chk = 0.f;
#pragma unroll
        for (int i = 0; i < 10 + CM; ++i) if (EXACT || i < 10 + C) { v[i] = d[i]; chk = fmaf(v[i], 0.f, chk); }
        if (chk != 0.f && p.status) atomicOr(p.status, 2u);
        float out[11 + CM];
        corners_(v[0], v[1], v[2], v[3], cell % p.lw, cell / p.lw, p.lw, p.lh, p.pw[pr], p.ph[pr], out);
        float prod = 1.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) { out[4 + i] = expf(v[4 + i]); }
        prod = ((out[4] * out[5]) * out[6]) * out[7];                   // tf.reduce_prod
        out[8] = prod;
        const float obj = sigmoidf_(v[8]);
        out[9] = obj;
        out[10] = logistic_entropy_(obj);
        softmax_<CM, EXACT>(v + 10, out + 11, C);
        const float clsH = softmax_entropy_<CM, EXACT>(out + 11, C);
        float* o = p.boxes + ((size_t)b * p.n_total + p.box_base + (size_t)pr * cells + cell) * D;
#pragma unroll
        for (int i = 0; i < 11 + CM; ++i) if (EXACT || i < 11 + C) o[i] = out[i];
        o[11 + C] = clsH;
        o[12 + C] = (float)p.layer_id;
        o[13 + C] = (float)pr;
    }
}

// 4x4 determinant by LU with partial pivoting (what tf.linalg.det does via Eigen PartialPivLU).
// The pivot row is swapped in with SELECTS over compile-time indices: a run-time row index (a[piv][c]) sends the matrix
// to scratch memory (20 bytes of private segment per lane in the first version), and this library's kernels stay out
// of scratch altogether -- kernels with private segments from several HIP streams at once disturbed each other's
// spilled values on this stack (tests/test_gpu_parity.py::test_engines_on_concurrent_streams: this determinant, whose
// value is rounding noise for T <= 4 samples, was the one visible symptom).
__device__ __forceinline__ float det4_(float a[4][4]) {
    float det = 1.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        int piv = k; float best = fabsf(a[k][k]);
#pragma unroll
        for (int r = k + 1; r < 4; ++r) { const float v = fabsf(a[r][k]); if (v > best) { best = v; piv = r; } }
#pragma unroll
        for (int r = k + 1; r < 4; ++r) {
            const bool sw = piv == r;                              // (same first-maximum choice, same swap as before)
#pragma unroll
            for (int c = 0; c < 4; ++c) { const float x = a[k][c], y = a[r][c]; a[k][c] = sw ? y : x; a[r][c] = sw ? x : y; }
        }
        if (piv != k) det = -det;
        const float d = a[k][k];
        det *= d;
        if (d != 0.f) {
#pragma unroll
            for (int r = k + 1; r < 4; ++r) {
                const float f = a[r][k] / d;
#pragma unroll
                for (int c = k + 1; c < 4; ++c) a[r][c] -= f * a[k][c];
            }
        }
    }
    return det;
}

// The finish of one row from a lane's running sums over its first Tf samples: means by division (see decode_epi_kernel on why),
// covariance, determinant, entropies and mutual informations, corners, layer / prior ids.  ONE copy: decode_epi_kernel (modes 0
// and 2) and decode_epi_ladder_kernel both end here, so a rung of the ladder cannot drift from the decode of the same samples.
template <int CM, bool EXACT>
__device__ __forceinline__ void epi_finish_(const DecodeParams& p, const float (&s_loc)[4], const float (&s_ll)[10], const float (&s_var)[4],
                                            float s_obj, float s_objH, const float (&s_cls)[CM], float s_clsH, float Tf, int C,
                                            int cell, int pr, float* o) {
    float ev[4], cov[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i) ev[i] = s_loc[i] / Tf;
    {
        int q = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = i; j < 4; ++j) {
                const float c = s_ll[q++] / Tf - ev[i] * ev[j];   // E[l l^T] - E[l]E[l]^T (layers.py:383)
                cov[i][j] = c; cov[j][i] = c;
            }
    }
    float out[17 + CM];
    corners_(ev[0], ev[1], ev[2], ev[3], cell % p.lw, cell / p.lw, p.lw, p.lh, p.pw[pr], p.ph[pr], out);
    float ale_sum = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        out[4 + i] = cov[i][i];
        const float a = s_var[i] / Tf;
        out[8 + i] = a;
        ale_sum += a;
    }
    out[12] = det4_(cov);
    out[13] = ale_sum;
    const float obj_mean = s_obj / Tf;
    const float objH = logistic_entropy_(obj_mean);
    out[14] = obj_mean;
    out[15] = objH - s_objH / Tf;
    out[16] = objH;
#pragma unroll
    for (int c = 0; c < CM; ++c) if (EXACT || c < C) out[17 + c] = s_cls[c] / Tf;
    const float clsH = softmax_entropy_<CM, EXACT>(out + 17, C);
#pragma unroll
    for (int i = 0; i < 17 + CM; ++i) if (EXACT || i < 17 + C) o[i] = out[i];
    o[17 + C] = clsH - s_clsH / Tf;
    o[18 + C] = clsH;
    o[19 + C] = (float)p.layer_id;
    o[20 + C] = (float)pr;
}

// One lane per (image, cell, prior): a single pass over the image's T samples keeps
// 4 + 10 + 4 + 1 + 1 + C + 1 running sums in registers.
template <int CM, bool EXACT>
__global__ __launch_bounds__(256) void decode_epi_kernel(const DecodeParams p) {
    const int C = EXACT ? CM : p.C;
    const int BLK = 2 * (5 + C), D = 21 + C;
    const int LDC = p.ld ? p.ld : 3 * BLK;
    const int cells = p.lh * p.lw;
    const int64_t total = (int64_t)p.B * cells * 3;
    const size_t sample_stride = (size_t)cells * LDC;
    // Every mean is the sum DIVIDED by T, as tf.reduce_mean forms it, not multiplied by a rounded 1 / T (tests/test_decode_f64_gpu.py):
    //  * `sum * invT` is up to an ulp of the mean off, and E[l l^T] - E[l] E[l]^T turns an ulp of E[l^2] into an absolute error: T = 7
    //    samples of a logit of 800 came out with a variance of -0.098 where the reference has 0 (5600 * fl(1 / 7) rounds to 800.00006);
    //  * a product can be contracted into what follows: `1 - s_obj * invT` became one fused multiply-add, so T = 50 samples of a
    //    saturated objectness (every sigmoid 1) had 1 - mean = 2.2e-8 beside a mean of 1, and the entropy 3.9e-7 where the reference
    //    has 0 * log 0 = NaN.  A quotient is rounded once and T / T is 1.
    const float Tf = (float)p.T;
    for (int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; gid < total;
         gid += (int64_t)gridDim.x * blockDim.x) {
        const int pr = (int)(gid % 3);
        const int64_t bc = gid / 3;
        const int cell = (int)(bc % cells), b = (int)(bc / cells);
        const float* d0 = p.raw + ((size_t)b * p.T) * sample_stride + (size_t)cell * LDC + pr * BLK;
        float s_loc[4] = {0, 0, 0, 0}, s_ll[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, s_var[4] = {0, 0, 0, 0};
        float s_obj = 0.f, s_objH = 0.f, s_cls[CM], s_clsH = 0.f;
        float chk = 0.f;                                        // stays 0 unless a raw value is inf / NaN
#pragma unroll
        for (int c = 0; c < CM; ++c) s_cls[c] = 0.f;
        float* o = p.boxes + ((size_t)b * p.n_total + p.box_base + (size_t)pr * cells + cell) * D;
        if (p.mode == 2) {                                      // the sums of ALL samples, added up across the ranks (byolo_finish_tshard)
#pragma unroll
            for (int i = 0; i < 4; ++i) { s_loc[i] = o[i]; s_var[i] = o[14 + i]; }
#pragma unroll
            for (int i = 0; i < 10; ++i) s_ll[i] = o[4 + i];
            s_obj = o[18]; s_objH = o[19];
#pragma unroll
            for (int c = 0; c < CM; ++c) if (EXACT || c < C) s_cls[c] = o[20 + c];
            s_clsH = o[20 + C];
        }
        for (int t = 0; t < (p.mode == 2 ? 0 : p.T); ++t) {
            const float* d = d0 + (size_t)t * sample_stride;
            float v[10 + CM];                                   // the two std logit groups are not decoded
#pragma unroll
            for (int i = 0; i < 10 + CM; ++i) if (EXACT || i < 10 + C) { v[i] = d[i]; chk = fmaf(v[i], 0.f, chk); }
            int q = 0;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                s_loc[i] += v[i];
                s_var[i] += expf(v[4 + i]);
#pragma unroll
                for (int j = i; j < 4; ++j) s_ll[q++] += v[i] * v[j];
            }
            const float obj = sigmoidf_(v[8]);
            s_obj += obj;
            s_objH += logistic_entropy_(obj);
            float pc[CM];
            softmax_<CM, EXACT>(v + 10, pc, C);
#pragma unroll
            for (int c = 0; c < CM; ++c) if (EXACT || c < C) s_cls[c] += pc[c];
            s_clsH += softmax_entropy_<CM, EXACT>(pc, C);
        }
        if (chk != 0.f && p.status) atomicOr(p.status, 2u);
        if (p.mode == 1) {                                      // this rank's share of the T samples: hand out the sums
#pragma unroll
            for (int i = 0; i < 4; ++i) { o[i] = s_loc[i]; o[14 + i] = s_var[i]; }
#pragma unroll
            for (int i = 0; i < 10; ++i) o[4 + i] = s_ll[i];
            o[18] = s_obj; o[19] = s_objH;
#pragma unroll
            for (int c = 0; c < CM; ++c) if (EXACT || c < C) o[20 + c] = s_cls[c];
            o[20 + C] = s_clsH;
            continue;
        }
        epi_finish_<CM, EXACT>(p, s_loc, s_ll, s_var, s_obj, s_objH, s_cls, s_clsH, Tf, C, cell, pr, o);
    }
}

// The MC sample-count ladder (include/byolo.h "MC sample-count ladder"): decode_epi_kernel's walk -- same lane mapping, loads and
// running sums -- taken rung by rung: t = 0 .. rungs[0] - 1, on to rungs[1] - 1, ..., and behind every rung the finish with
// Tf = rungs[k].  After k samples the sums ARE what a T = k reduction of the image's first k samples holds, so rung k's row, written
// into slab k (boxes + k * slab_stride, inside the slab at decode_epi_kernel's position), is decode_epi_kernel's row of those
// samples.  The image stride of `raw` stays p.T samples whatever the rungs are, and the walk ends at the last rung.  The rung loop is
// uniform across the launch, and the rungs are read from the kernel arguments only (scalar loads at a uniform index): nothing goes
// to scratch.  Builds up to 48 class slots (the 128-slot build of the other decode kernels spills; tests/test_no_scratch.py exempts
// only those): launch_decode_ladder refuses more.
//
// BIT FOR BIT is the contract, and sharing epi_finish_ is not enough for it.  Under -ffp-contract=fast the compiler decides per basic
// block which product of a sum of two it fuses -- H = -(a log a + b log b) has two candidates -- after the SLP vectoriser has paired
// the running sums, and it pairs them by where they are loaded and stored: decode_epi_kernel's T-shard paths (p.mode 1 and 2) among
// them.  A walk without those paths, or without the check of the raw values, came out an ulp off in the summed entropies in most
// builds (the mutual informations of a single sample were 0 in one kernel and 6e-8 in the other).  So the per-lane body below is
// decode_epi_kernel's statement for statement, the sum load / store paths and `chk` included, although launch_decode_ladder admits
// mode 0 only and its callers pass no status word (the forward's own decode has looked at the same raw values): they are never
// taken.  tests/test_t_ladder_gpu.py holds every build to the decode, and profiles/t_ladder.md says how far the two kernels' machine
// code agrees.  Change the walk of one kernel and the other must follow.
template <int CM, bool EXACT>
__global__ __launch_bounds__(256) void decode_epi_ladder_kernel(const DecodeParams p, const LadderParams r) {
    const int C = EXACT ? CM : p.C;
    const int BLK = 2 * (5 + C), D = 21 + C;
    const int LDC = p.ld ? p.ld : 3 * BLK;
    const int cells = p.lh * p.lw;
    const int64_t total = (int64_t)p.B * cells * 3;
    const size_t sample_stride = (size_t)cells * LDC;
    for (int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; gid < total;
         gid += (int64_t)gridDim.x * blockDim.x) {
        const int pr = (int)(gid % 3);
        const int64_t bc = gid / 3;
        const int cell = (int)(bc % cells), b = (int)(bc / cells);
        const float* d0 = p.raw + ((size_t)b * p.T) * sample_stride + (size_t)cell * LDC + pr * BLK;
        float s_loc[4] = {0, 0, 0, 0}, s_ll[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, s_var[4] = {0, 0, 0, 0};
        float s_obj = 0.f, s_objH = 0.f, s_cls[CM], s_clsH = 0.f;
        float chk = 0.f;
#pragma unroll
        for (int c = 0; c < CM; ++c) s_cls[c] = 0.f;
        float* o = p.boxes + ((size_t)b * p.n_total + p.box_base + (size_t)pr * cells + cell) * D;
        if (p.mode == 2) {                                      // (never taken: see above)
#pragma unroll
            for (int i = 0; i < 4; ++i) { s_loc[i] = o[i]; s_var[i] = o[14 + i]; }
#pragma unroll
            for (int i = 0; i < 10; ++i) s_ll[i] = o[4 + i];
            s_obj = o[18]; s_objH = o[19];
#pragma unroll
            for (int c = 0; c < CM; ++c) if (EXACT || c < C) s_cls[c] = o[20 + c];
            s_clsH = o[20 + C];
        }
        int t = 0;
        for (int k = 0; k < r.n_rungs; ++k) {                   // (uniform: every lane of the launch walks the same rungs)
            const int next = r.rungs[k];
            for (; t < next; ++t) {
                const float* d = d0 + (size_t)t * sample_stride;
                float v[10 + CM];                               // the two std logit groups are not decoded
#pragma unroll
                for (int i = 0; i < 10 + CM; ++i) if (EXACT || i < 10 + C) { v[i] = d[i]; chk = fmaf(v[i], 0.f, chk); }
                int q = 0;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    s_loc[i] += v[i];
                    s_var[i] += expf(v[4 + i]);
#pragma unroll
                    for (int j = i; j < 4; ++j) s_ll[q++] += v[i] * v[j];
                }
                const float obj = sigmoidf_(v[8]);
                s_obj += obj;
                s_objH += logistic_entropy_(obj);
                float pc[CM];
                softmax_<CM, EXACT>(v + 10, pc, C);
#pragma unroll
                for (int c = 0; c < CM; ++c) if (EXACT || c < C) s_cls[c] += pc[c];
                s_clsH += softmax_entropy_<CM, EXACT>(pc, C);
            }
            if (p.mode == 1) {                                  // (never taken: see above)
#pragma unroll
                for (int i = 0; i < 4; ++i) { o[i] = s_loc[i]; o[14 + i] = s_var[i]; }
#pragma unroll
                for (int i = 0; i < 10; ++i) o[4 + i] = s_ll[i];
                o[18] = s_obj; o[19] = s_objH;
#pragma unroll
                for (int c = 0; c < CM; ++c) if (EXACT || c < C) o[20 + c] = s_cls[c];
                o[20 + C] = s_clsH;
                o += r.slab_stride;
                continue;
            }
            epi_finish_<CM, EXACT>(p, s_loc, s_ll, s_var, s_obj, s_objH, s_cls, s_clsH, (float)next, C, cell, pr, o);
            o += r.slab_stride;
        }
        if (chk != 0.f && p.status) atomicOr(p.status, 2u);
    }
}

// The entries of decode_epistemic's dict (lib_yolo/layers.py:397-411) that are not columns of the box row: the mean
// raw location logits `ev_loc`, the full 4x4 `epi_covar_loc` (same one-pass sums as decode_epi_kernel: its diagonal
// equals the row's columns 4..7 bit for bit) and the per-sample `obj_samples` / `cls_samples`.  One lane per
// (image, cell, prior); any output may be null.
template <int CM, bool EXACT>
__global__ __launch_bounds__(256) void epi_stats_kernel(const DecodeParams p, float* ev_loc, float* covar, float* obj_s, float* cls_s) {
    const int C = EXACT ? CM : p.C;
    const int BLK = 2 * (5 + C);
    const int LDC = p.ld ? p.ld : 3 * BLK;
    const int cells = p.lh * p.lw;
    const int64_t total = (int64_t)p.B * cells * 3;
    const size_t sample_stride = (size_t)cells * LDC;
    const float Tf = (float)p.T;                                  // divided, not multiplied by 1 / T: see decode_epi_kernel
    for (int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; gid < total;
         gid += (int64_t)gridDim.x * blockDim.x) {
        const int pr = (int)(gid % 3);
        const int64_t bc = gid / 3;
        const int cell = (int)(bc % cells), b = (int)(bc / cells);
        const float* d0 = p.raw + ((size_t)b * p.T) * sample_stride + (size_t)cell * LDC + pr * BLK;
        float s_loc[4] = {0, 0, 0, 0}, s_ll[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        for (int t = 0; t < p.T; ++t) {
            const float* d = d0 + (size_t)t * sample_stride;
            float v[10 + CM];
#pragma unroll
            for (int i = 0; i < 10 + CM; ++i) if (EXACT || i < 10 + C) v[i] = d[i];
            int q = 0;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                s_loc[i] += v[i];
#pragma unroll
                for (int j = i; j < 4; ++j) s_ll[q++] += v[i] * v[j];
            }
            const size_t so = (((size_t)b * p.T + t) * cells + cell) * 3 + pr;       // [S, lh, lw, 3]
            if (obj_s) obj_s[so] = sigmoidf_(v[8]);
            if (cls_s) {
                float pc[CM];
                softmax_<CM, EXACT>(v + 10, pc, C);
#pragma unroll
                for (int c = 0; c < CM; ++c) if (EXACT || c < C) cls_s[so * C + c] = pc[c];
            }
        }
        float ev[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) ev[i] = s_loc[i] / Tf;
        const size_t o = ((size_t)b * cells + cell) * 3 + pr;                        // [B, lh, lw, 3]
        if (ev_loc) {
#pragma unroll
            for (int i = 0; i < 4; ++i) ev_loc[o * 4 + i] = ev[i];
        }
        if (covar) {
            int q = 0;
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = i; j < 4; ++j) {
                    const float c = s_ll[q++] / Tf - ev[i] * ev[j];                // E[l l^T] - E[l]E[l]^T (layers.py:383)
                    covar[o * 16 + i * 4 + j] = c; covar[o * 16 + j * 4 + i] = c;
                }
        }
    }
}

template <int CM, bool EXACT>
static hipError_t launch_epi_stats_c(const DecodeParams& p, float* ev, float* cov, float* os, float* cs, hipStream_t st) {
    const int64_t total = (int64_t)p.B * p.lh * p.lw * 3;
    const int64_t blocks = std::max<int64_t>(1, std::min<int64_t>(4096, (total + 255) / 256));
    hipLaunchKernelGGL((epi_stats_kernel<CM, EXACT>), dim3((unsigned)blocks), dim3(256), 0, st, p, ev, cov, os, cs);
    return hipGetLastError();
}

hipError_t launch_epi_stats(const DecodeParams& p, float* ev, float* cov, float* os, float* cs, hipStream_t st) {
    if (p.C < 1 || p.C > BYOLO_MAX_CLASSES) return hipErrorInvalidValue;
    if (p.C == 2) return launch_epi_stats_c<2, true>(p, ev, cov, os, cs, st);
    if (p.C <= 8) return launch_epi_stats_c<8, false>(p, ev, cov, os, cs, st);
    if (p.C <= 24) return launch_epi_stats_c<24, false>(p, ev, cov, os, cs, st);
    if (p.C <= 48) return launch_epi_stats_c<48, false>(p, ev, cov, os, cs, st);
    return launch_epi_stats_c<BYOLO_MAX_CLASSES, false>(p, ev, cov, os, cs, st);
}

template <int CM, bool EXACT>
static hipError_t launch_decode_c(int kind, const DecodeParams& p, hipStream_t st) {
    const int64_t total = (int64_t)p.B * p.lh * p.lw * 3;
    int64_t blocks = (total + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    if (blocks < 1) blocks = 1;
    if (kind == 0) hipLaunchKernelGGL((decode_std_kernel<CM, EXACT>), dim3((unsigned)blocks), dim3(256), 0, st, p);
    else if (kind == 1) hipLaunchKernelGGL((decode_ale_kernel<CM, EXACT>), dim3((unsigned)blocks), dim3(256), 0, st, p);
    else hipLaunchKernelGGL((decode_epi_kernel<CM, EXACT>), dim3((unsigned)blocks), dim3(256), 0, st, p);
    return hipGetLastError();
}

// The reference takes any cls_cnt (lib_yolo/yolov3.py:180): exact builds for the usual counts, capacity builds
// (slots masked by the runtime count; the large ones spill to scratch -- correct, not fast) for everything else.
hipError_t launch_decode(int kind, const DecodeParams& p, hipStream_t st) {
    switch (p.C) {
        case 1: return launch_decode_c<1, true>(kind, p, st);
        case 2: return launch_decode_c<2, true>(kind, p, st);
        case 3: return launch_decode_c<3, true>(kind, p, st);
        case 4: return launch_decode_c<4, true>(kind, p, st);
        case 8: return launch_decode_c<8, true>(kind, p, st);
        case 80: return launch_decode_c<80, true>(kind, p, st);
        default: break;
    }
    if (p.C < 1 || p.C > BYOLO_MAX_CLASSES) return hipErrorInvalidValue;
    if (p.C <= 8) return launch_decode_c<8, false>(kind, p, st);
    if (p.C <= 24) return launch_decode_c<24, false>(kind, p, st);
    if (p.C <= 48) return launch_decode_c<48, false>(kind, p, st);
    return launch_decode_c<BYOLO_MAX_CLASSES, false>(kind, p, st);
}

template <int CM, bool EXACT>
static hipError_t launch_decode_ladder_c(const DecodeParams& p, const LadderParams& r, hipStream_t st) {
    const int64_t total = (int64_t)p.B * p.lh * p.lw * 3;
    const int64_t blocks = std::max<int64_t>(1, std::min<int64_t>(4096, (total + 255) / 256));
    hipLaunchKernelGGL((decode_epi_ladder_kernel<CM, EXACT>), dim3((unsigned)blocks), dim3(256), 0, st, p, r);
    return hipGetLastError();
}

// The exact and capacity builds of launch_decode below the 128-slot one; what the callers have checked is checked again, because
// a rung outside 1 .. T walks past the end of `raw`.
hipError_t launch_decode_ladder(const DecodeParams& p, const LadderParams& r, hipStream_t st) {
    if (p.C < 1 || p.C > T_LADDER_MAX_CLASSES || p.mode != 0 || r.n_rungs < 1 || r.n_rungs > T_LADDER_MAX) return hipErrorInvalidValue;
    for (int k = 0; k < r.n_rungs; ++k)
        if (r.rungs[k] < (k ? r.rungs[k - 1] + 1 : 1) || r.rungs[k] > p.T) return hipErrorInvalidValue;
    switch (p.C) {
        case 1: return launch_decode_ladder_c<1, true>(p, r, st);
        case 2: return launch_decode_ladder_c<2, true>(p, r, st);
        case 3: return launch_decode_ladder_c<3, true>(p, r, st);
        case 4: return launch_decode_ladder_c<4, true>(p, r, st);
        case 8: return launch_decode_ladder_c<8, true>(p, r, st);
        default: break;
    }
    if (p.C <= 8) return launch_decode_ladder_c<8, false>(p, r, st);
    if (p.C <= 24) return launch_decode_ladder_c<24, false>(p, r, st);
    return launch_decode_ladder_c<48, false>(p, r, st);
}

// ------------------------------------------------------------------------------------------------
// K8 / K9: score order, greedy NMS and gather.  One pipeline serves every mode (the pc_* kernels at the end of this
// file); what follows first are the device functions its kernels share.  A sort key is 64 bits, (score key, row index):
// ascending keys == (score descending, index ascending), the order TensorFlow's kernel visits the boxes in.
// ------------------------------------------------------------------------------------------------
// (score_key: nms_box.h -- the vote stage of box_vote.hip decides "candidate" with the same function)
__device__ __forceinline__ void ce(unsigned long long& a, unsigned long long& b, bool up) {
    if ((a > b) == up) { const unsigned long long t = a; a = b; b = t; }
}

// ------------------------------------------------------------------------------------------------
// The exact walk (pc_general_kernel): one 1024-thread workgroup per class of an image, candidates in sorted order,
// 1024 per round:
//   phase A  every lane tests its candidate against all boxes kept in earlier rounds (LDS broadcast)
//   phase B  the 16 waves take turns: intra-wave 64x64 suppression bit-matrix, serial resolve over
//            the 64 candidates with readlane, kept boxes appended to the LDS list, the later waves
//            then test against just those.
// IoU is evaluated operation-for-operation as TensorFlow's IOU() in float32 with single rounding
// (__f*_rn: no FMA contraction), std::min/std::max NaN semantics -> kept indices bit-exact.
// ------------------------------------------------------------------------------------------------
static constexpr int NMS_THREADS = 1024;
static constexpr int NMS_MAXK = 2048;                        // max_out limit per class

// LDS of one walk: the kept boxes so far, the staging of the wave whose turn it is, the kept count.
struct WalkLds {
    float k_y0[NMS_MAXK], k_x0[NMS_MAXK], k_y1[NMS_MAXK], k_x1[NMS_MAXK], k_ar[NMS_MAXK];
    float w_y0[64], w_x0[64], w_y1[64], w_x1[64], w_ar[64];
    int s_nk;
};

// One greedy pass of the whole workgroup over the score-ordered `keys[0 .. n_valid)`: emit(pos, idx) receives the
// pos-th kept box.  Returns the number kept (uniform).
template <class Emit>
__device__ __forceinline__ int greedy_walk(WalkLds& L, const float* bx, int D, const unsigned long long* keys, int n_valid,
                                           int max_out, float thr, Emit emit) {
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    if (tid == 0) L.s_nk = 0;
    __syncthreads();
    int nk_cur = 0;                                          // register copy of s_nk, uniform across the block
    for (int base = 0; base < n_valid && nk_cur < max_out; base += NMS_THREADS) {
        const int i = base + tid;
        bool alive = i < n_valid;
        int idx = -1;
        NBox me = {0, 0, 0, 0, 0};
        if (alive) {
            idx = (int)(keys[i] & 0xFFFFFFFFull);
            const float* r = bx + (size_t)idx * D;
            me = make_box(r[0], r[1], r[2], r[3]);
        }
        // phase A: against everything kept in earlier rounds
        for (int k = 0; k < nk_cur; ++k) {
            if (alive) {
                const NBox kb = {L.k_y0[k], L.k_x0[k], L.k_y1[k], L.k_x1[k], L.k_ar[k]};
                if (iou_gt(me, kb, thr)) alive = false;
            }
        }
        // phase B: the 16 waves take turns
        for (int sub = 0; sub < NMS_THREADS / 64 && nk_cur < max_out; ++sub) {
            if (wave == sub) {
                const unsigned long long alive_mask = __ballot(alive);
                if (alive_mask) {
                    L.w_y0[lane] = me.y0; L.w_x0[lane] = me.x0; L.w_y1[lane] = me.y1; L.w_x1[lane] = me.x1; L.w_ar[lane] = me.area;
                    unsigned long long supp = 0ull;          // bit e: earlier live candidate e overlaps me
                    for (int e = 0; e < 64; ++e) {
                        if (e < lane && ((alive_mask >> e) & 1ull) && alive) {
                            const NBox ob = {L.w_y0[e], L.w_x0[e], L.w_y1[e], L.w_x1[e], L.w_ar[e]};
                            if (iou_gt(me, ob, thr)) supp |= (1ull << e);
                        }
                    }
                    const unsigned int supp_lo = (unsigned int)supp, supp_hi = (unsigned int)(supp >> 32);
                    unsigned long long keptmask = 0ull;
                    int room = max_out - nk_cur;
                    for (int e = 0; e < 64 && room > 0; ++e) {           // serial greedy resolve (uniform)
                        if ((alive_mask >> e) & 1ull) {
                            const unsigned long long se =
                                ((unsigned long long)(unsigned int)__builtin_amdgcn_readlane((int)supp_hi, e) << 32) |
                                (unsigned int)__builtin_amdgcn_readlane((int)supp_lo, e);
                            if ((se & keptmask) == 0ull) { keptmask |= (1ull << e); --room; }
                        }
                    }
                    if ((keptmask >> lane) & 1ull) {
                        const int pos = nk_cur + __popcll(keptmask & ((1ull << lane) - 1ull));
                        L.k_y0[pos] = me.y0; L.k_x0[pos] = me.x0; L.k_y1[pos] = me.y1; L.k_x1[pos] = me.x1; L.k_ar[pos] = me.area;
                        emit(pos, idx);
                    }
                    if (lane == 0) L.s_nk = nk_cur + __popcll(keptmask);
                }
            }
            __syncthreads();
            const int nk_new = L.s_nk;
            if (wave > sub && alive) {
                for (int k = nk_cur; k < nk_new; ++k) {
                    const NBox kb = {L.k_y0[k], L.k_x0[k], L.k_y1[k], L.k_x1[k], L.k_ar[k]};
                    if (iou_gt(me, kb, thr)) { alive = false; break; }
                }
            }
            nk_cur = nk_new;
            __syncthreads();                                 // nobody still reads s_nk / w_* when the next wave writes
        }
    }
    return nk_cur;
}

// ------------------------------------------------------------------------------------------------
// The prefix path: greedy NMS only ever looks at a PREFIX of the score order (until max_out boxes are kept), and on
// that prefix it is a bit-matrix problem that the whole chip can work on:
//   matrix_tile   suppression bit matrix of the sorted prefix (row r, bit c: c later than r and IoU > thr), in 64 x 64
//                 tiles, upper triangle only
//   scan_prefix   serial greedy scan over the prefix, 64 candidates per step from LDS, the 4096-bit "removed" set
//                 lives in one wave's registers (lane w = word w)
// Same result as the sequential definition.  If the prefix is exhausted before max_out boxes are kept while more
// candidates exist (pathological clustering), or scores tie en masse, the class is flagged and the exact walk above
// redoes it after a full sort -- decided on the device, no host round trip.
// ------------------------------------------------------------------------------------------------
static constexpr int NMS_TOPK = 4096;                        // prefix length / matrix dimension
static constexpr int NMS_CAP = 8192;                         // LDS sort capacity (prefix + score ties)
static constexpr int NMS_WORDS = NMS_TOPK / 64;

// One 64 x 64 tile of a suppression matrix: rows rb*64.., bit columns w*64.. of the Kc-long sorted prefix `cand`;
// `mask` holds NMS_WORDS words per row.  One wave.
__device__ __forceinline__ void matrix_tile(const float* bx, int D, float thr, const unsigned long long* cand, int Kc,
                                            int rb, int w, unsigned long long* mask) {
    __shared__ float c_y0[64], c_x0[64], c_y1[64], c_x1[64], c_ar[64];
    const int lane = threadIdx.x;
    const int r = rb * 64 + lane, c = w * 64 + lane;
    NBox me = {0, 0, 0, 0, 0};
    if (r < Kc) { const float* q = bx + (size_t)(cand[r] & 0xFFFFFFFFull) * D; me = make_box(q[0], q[1], q[2], q[3]); }
    if (c < Kc) {
        const float* q = bx + (size_t)(cand[c] & 0xFFFFFFFFull) * D;
        const NBox o = make_box(q[0], q[1], q[2], q[3]);
        c_y0[lane] = o.y0; c_x0[lane] = o.x0; c_y1[lane] = o.y1; c_x1[lane] = o.x1; c_ar[lane] = o.area;
    }
    __syncthreads();
    unsigned long long bits = 0ull;
    if (r < Kc) {
        for (int e = 0; e < 64; ++e) {
            const int col = w * 64 + e;
            if (col > r && col < Kc) {
                const NBox o = {c_y0[e], c_x0[e], c_y1[e], c_x1[e], c_ar[e]};
                if (iou_gt(me, o, thr)) bits |= 1ull << e;
            }
        }
        mask[(size_t)r * NMS_WORDS + w] = bits;
    }
}

// Serial greedy scan of one sorted prefix (`cand`, n_cand keys, its matrix `mask`) by one 256-thread workgroup:
// kept indices to `kidx`, their number to *cnt, *need = 1 where the prefix cannot prove the result.
__device__ __forceinline__ void scan_prefix(int max_out, const unsigned long long* cand, int n_cand, const int* more,
                                            const unsigned long long* mask, int* kidx, int* cnt, int* need) {
    // The 64 matrix rows of a step, double-buffered (2 x 32 KiB, dynamic LDS): waves 1..3 fetch the rows of step c+1
    // while wave 0 resolves step c -- the fetch latency (L2) leaves the serial chain.
    extern __shared__ __attribute__((aligned(16))) unsigned long long rows_all[];   // [2][64][NMS_WORDS]
    __shared__ int s_nk, s_done;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int Kc = n_cand > NMS_TOPK ? NMS_TOPK : n_cand;
    const int nwords = (Kc + 63) / 64;
    if (tid == 0) { s_nk = 0; s_done = 0; }
    auto fetch = [&](int c, int first, int nthreads) {       // rows of step c -> buffer c & 1, by `nthreads` threads from `first`
        unsigned long long (*rows)[NMS_WORDS] = reinterpret_cast<unsigned long long (*)[NMS_WORDS]>(rows_all + (size_t)(c & 1) * 64 * NMS_WORDS);
        for (int t = tid - first; t < 64 * NMS_WORDS; t += nthreads) {
            const int r = t / NMS_WORDS, w = t - r * NMS_WORDS;
            const int gi = c * 64 + r;
            rows[r][w] = (w >= c && w < nwords && gi < Kc) ? mask[(size_t)gi * NMS_WORDS + w] : 0ull;
        }
    };
    unsigned long long rem = 0ull;                           // wave 0, lane w: word w of the removed set
    if (nwords > 0) fetch(0, 0, 256);
    __syncthreads();
    for (int c = 0; c < nwords; ++c) {
        if (wave != 0) {
            if (c + 1 < nwords) fetch(c + 1, 64, 192);
        } else {
            const unsigned long long (*rows)[NMS_WORDS] = reinterpret_cast<const unsigned long long (*)[NMS_WORDS]>(rows_all + (size_t)(c & 1) * 64 * NMS_WORDS);
            // The only serial dependency is the removed-word of THIS step (`cur`); everything on its
            // chain stays in registers: lane i holds word c of row i (suppression inside the step) and
            // candidate i's box index.  Folding the kept rows into the other 63 words of the removed set
            // and writing the kept indices happen after the loop, fully parallel.
            const int nk0 = s_nk;
            const int gi_l = c * 64 + lane;
            const unsigned long long own = rows[lane][c];
            const int my_idx = gi_l < Kc ? (int)(cand[gi_l] & 0xFFFFFFFFull) : -1;
            const unsigned int own_lo = (unsigned int)own, own_hi = (unsigned int)(own >> 32);
            unsigned long long cur =
                ((unsigned long long)(unsigned int)__builtin_amdgcn_readlane((int)(rem >> 32), c) << 32) |
                (unsigned int)__builtin_amdgcn_readlane((int)(unsigned int)rem, c);
            unsigned long long keptmask = 0ull;
            int nk = nk0;
            const int lim = Kc - c * 64 < 64 ? Kc - c * 64 : 64;
            if (lim < 64) cur |= ~0ull << lim;               // positions past the last candidate are never kept
            // visit only the survivors: the next candidate that is not suppressed = the lowest clear bit of `cur`
            // at or above the last kept one (a suppressed run costs nothing)
            unsigned long long done = 0ull;                  // bits below the scan position
            while (nk < max_out) {
                const unsigned long long open = ~(cur | done);
                if (!open) break;
                const int i = __builtin_ctzll(open);
                keptmask |= 1ull << i;
                ++nk;
                cur |= ((unsigned long long)(unsigned int)__builtin_amdgcn_readlane((int)own_hi, i) << 32) |
                       (unsigned int)__builtin_amdgcn_readlane((int)own_lo, i);
                done = (i == 63) ? ~0ull : ((2ull << i) - 1ull);
            }
            if ((keptmask >> lane) & 1ull) kidx[nk0 + __popcll(keptmask & ((1ull << lane) - 1ull))] = my_idx;
            // fold the kept rows into the removed set: 64 independent LDS reads per lane, selected by the kept bit
            unsigned long long acc = 0ull;
#pragma unroll 16
            for (int i = 0; i < 64; ++i) acc |= ((keptmask >> i) & 1ull) ? rows[i][lane] : 0ull;
            rem |= acc;
            if (lane == 0) { s_nk = nk; s_done = nk >= max_out ? 1 : 0; }
        }
        __syncthreads();
        if (s_done) break;
    }
    if (tid == 0) {
        const int nk = s_nk;
        *cnt = nk;
        // prefix exhausted without filling max_out although more candidates exist -> general path
        if (nk < max_out && (*more || n_cand > Kc)) *need = 1;
    }
}

// ------------------------------------------------------------------------------------------------
// The NMS pipeline of every mode: one NMS per class, the classes of an image side by side.  The modes differ in the class
// count C alone (NmsParams::C): BYOLO_NMS_AGNOSTIC is one class that every candidate row belongs to (no class column is
// read), BYOLO_NMS_TWO_CLASS two, BYOLO_NMS_PER_CLASS the model's cls_cnt.
//   pc_classify   every row: its class (the strict unique maximum of the C class scores, else none) as one byte --
//                 the digit above the score bits of the sort key -- and the per-image class histogram (two kernels:
//                 rows read in place for few classes, class scores staged through LDS for many)
//   pc_offsets    per image: segment / matrix-row / tile offsets of the classes (prefix sums of the histogram)
//   pc_scatter    counting sort on the class digit: (score key, index) of every member into its class segment
//   pc_select     grid (class, image): sorted prefix of the segment -- the whole segment where it fits LDS (NMS_CAP),
//                 else a 3-level radix select (11 + 11 + 10 bits of the score key) of the best >= NMS_TOPK keys, then
//                 compaction and a bitonic sort in LDS
//   pc_matrix     the 64 x 64 tiles of all classes' suppression matrices, as one linear list per image
//   pc_scan       grid (class, image): scan_prefix; a class whose prefix cannot prove its result sets need[b][c]
//   pc_general    grid (class, image), flagged classes only: full sort of the segment + greedy_walk
//   pc_finish     kept rows of class 0, 1, ... back to back, zero fill, counts
// An empty class costs one workgroup that reads its length and returns, in every stage.
// ------------------------------------------------------------------------------------------------
static_assert(BYOLO_MAX_CLASSES < PC_NONE, "the class digit of the per-class NMS key is one byte");
static constexpr int PC_ROWS = 128;                          // output rows per pc_finish workgroup
static constexpr int PC_TILE = 64;                           // rows per pc_classify_tiled workgroup
static constexpr int PC_DIRECT_C = 8;                        // up to this many classes pc_classify reads the rows in place

struct PcWs {
    unsigned char* cls;                                      // [B][N]
    int *hist, *cursor;                                      // [B][C+1] members per class (slot C unused), scatter cursors
    int *seg_off, *row_off, *tile_off;                       // [B][C+1] exclusive prefix sums
    int *n_cand, *more, *need;                               // [B][C+1]
    int* cnt;                                                // [B][C] kept per class
    unsigned long long *seg, *cand;                          // [B][N] keys by class segment: unordered / sorted prefix
    unsigned long long* mask;                                // [B][R][NMS_WORDS], R = pc_mask_rows
    int* kidx;                                               // [B][C][NMS_MAXK]
};
static inline int64_t pc_mask_rows(int64_t N, int C) { return std::min<int64_t>(N, (int64_t)C * NMS_TOPK); }
static inline int64_t pc_max_tiles(int64_t N, int C) {       // sum of T(T+1)/2 over classes, T <= 64, sum T <= N/64 + C
    return std::min<int64_t>((int64_t)C * (NMS_WORDS * (NMS_WORDS + 1) / 2), (N / 64 + C) * (NMS_WORDS + 1) / 2 + 1);
}
static size_t pc_ws_layout(int B, int64_t N, int C, char* base, PcWs* w) {
    size_t o = 0;
    auto take = [&](size_t bytes) { char* p = base ? base + o : nullptr; o += (bytes + 255) / 256 * 256; return p; };
    const size_t ci = (size_t)B * (C + 1) * 4;
    char* hc = take(2 * ci);                                 // hist + cursor: cleared by one launch_zero_words
    char* so = take(ci); char* ro = take(ci); char* to = take(ci); char* nc = take(ci); char* mo = take(ci); char* ne = take(ci);
    char* cn = take((size_t)B * C * 4);
    char* cl = take((size_t)B * N);
    char* sg = take((size_t)B * N * 8); char* cd = take((size_t)B * N * 8);
    char* mk = take((size_t)B * pc_mask_rows(N, C) * NMS_WORDS * 8);
    char* ki = take((size_t)B * C * NMS_MAXK * 4);
    if (w) { w->hist = (int*)hc; w->cursor = (int*)(hc ? hc + ci : nullptr); w->seg_off = (int*)so; w->row_off = (int*)ro;
             w->tile_off = (int*)to; w->n_cand = (int*)nc; w->more = (int*)mo; w->need = (int*)ne; w->cnt = (int*)cn;
             w->cls = (unsigned char*)cl; w->seg = (unsigned long long*)sg; w->cand = (unsigned long long*)cd;
             w->mask = (unsigned long long*)mk; w->kidx = (int*)ki; }
    return o;
}
const int32_t* nms_class_counts_ptr(void* ws, int B, int64_t N, int C) {
    PcWs w;
    pc_ws_layout(B, N, C, reinterpret_cast<char*>(ws), &w);
    return w.cnt;
}
size_t nms_workspace_bytes(int B, int64_t N, int C) { return pc_ws_layout(B, N, C, nullptr, nullptr); }   // grows with C

// (classify_row: nms_box.h, shared with box_vote.hip)
// Few classes (C <= PC_DIRECT_C): one lane per row reads its class scores where they are.
__global__ __launch_bounds__(256) void pc_classify_kernel(const float* boxes, int64_t N, int D, int obj_idx, int cls_start,
                                                          int C, unsigned char* cls_all, int* hist_all) {
    __shared__ int h[PC_DIRECT_C];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * 256 + tid;
    if (tid < C) h[tid] = 0;
    __syncthreads();
    if (i < N) {
        const float* r = boxes + ((size_t)b * N + i) * D;
        const int cl = classify_row(r + cls_start, C, r[obj_idx]);
        cls_all[(size_t)b * N + i] = (unsigned char)cl;
        if (cl != PC_NONE) atomicAdd(&h[cl], 1);
    }
    __syncthreads();
    if (tid < C && h[tid]) atomicAdd(&hist_all[(size_t)b * (C + 1) + tid], h[tid]);
}

// Many classes: the class scores of PC_TILE rows go through LDS -- the workgroup reads each row's C columns with consecutive
// lanes, then one lane per row scans them (row stride odd: no bank conflict).  Lanes that walk wide rows of their own in global
// memory touch 64 cache lines per load and evict each other's lines before the next column is read (C = 80: 1.7 ms for
// 11 x 120 960 rows that way).
__global__ __launch_bounds__(256) void pc_classify_tiled_kernel(const float* boxes, int64_t N, int D, int obj_idx, int cls_start,
                                                                int C, unsigned char* cls_all, int* hist_all) {
    __shared__ float tile[PC_TILE * (BYOLO_MAX_CLASSES + 1)];
    __shared__ int h[BYOLO_MAX_CLASSES];
    const int b = blockIdx.y, tid = threadIdx.x, S = C | 1;
    const int64_t i0 = (int64_t)blockIdx.x * PC_TILE;
    const int nrow = N - i0 < PC_TILE ? (int)(N - i0) : PC_TILE;
    const float* bx = boxes + ((size_t)b * N + i0) * D;
    for (int c = tid; c < C; c += 256) h[c] = 0;
    for (int e = tid; e < nrow * C; e += 256) {
        const int r = e / C, c = e - r * C;
        tile[r * S + c] = bx[(size_t)r * D + cls_start + c];
    }
    __syncthreads();
    if (tid < nrow) {
        const int cl = classify_row(tile + tid * S, C, bx[(size_t)tid * D + obj_idx]);
        cls_all[(size_t)b * N + i0 + tid] = (unsigned char)cl;
        if (cl != PC_NONE) atomicAdd(&h[cl], 1);
    }
    __syncthreads();
    for (int c = tid; c < C; c += 256)
        if (h[c]) atomicAdd(&hist_all[(size_t)b * (C + 1) + c], h[c]);
}

__global__ __launch_bounds__(64) void pc_offsets_kernel(int C, int general_only, PcWs w) {
    __shared__ int hist[BYOLO_MAX_CLASSES];
    const int b = blockIdx.x, tid = threadIdx.x, CS = C + 1;
    for (int c = tid; c < C; c += 64) {
        hist[c] = w.hist[(size_t)b * CS + c];
        w.n_cand[(size_t)b * CS + c] = 0; w.more[(size_t)b * CS + c] = 0; w.need[(size_t)b * CS + c] = general_only;
        w.cnt[(size_t)b * C + c] = 0;
    }
    __syncthreads();
    if (tid == 0) {
        int so = 0, ro = 0, to = 0;
        for (int c = 0; c <= C; ++c) {
            w.seg_off[(size_t)b * CS + c] = so; w.row_off[(size_t)b * CS + c] = ro; w.tile_off[(size_t)b * CS + c] = to;
            if (c == C) break;
            const int n = hist[c], kc = n < NMS_TOPK ? n : NMS_TOPK, t = (kc + 63) / 64;
            so += n; ro += kc; to += t * (t + 1) / 2;
        }
    }
}

__global__ __launch_bounds__(256) void pc_scatter_kernel(const float* boxes, int64_t N, int D, int obj_idx, int C, PcWs w) {
    __shared__ int h[BYOLO_MAX_CLASSES], base[BYOLO_MAX_CLASSES];
    const int b = blockIdx.y, tid = threadIdx.x, CS = C + 1;
    const int64_t i = (int64_t)blockIdx.x * 256 + tid;
    for (int c = tid; c < C; c += 256) h[c] = 0;
    __syncthreads();
    const int cl = i < N ? (int)w.cls[(size_t)b * N + i] : PC_NONE;
    int rank = -1;
    if (cl != PC_NONE) rank = atomicAdd(&h[cl], 1);
    __syncthreads();
    for (int c = tid; c < C; c += 256)
        if (h[c]) base[c] = w.seg_off[(size_t)b * CS + c] + atomicAdd(&w.cursor[(size_t)b * CS + c], h[c]);
    __syncthreads();
    if (rank >= 0) {
        const unsigned int k = score_key(boxes[((size_t)b * N + i) * D + obj_idx]);
        w.seg[(size_t)b * N + base[cl] + rank] = ((unsigned long long)k << 32) | (unsigned int)i;
    }
}

__global__ __launch_bounds__(1024) void pc_select_kernel(int64_t N, int C, PcWs w) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long sbuf[];      // NMS_CAP keys
    __shared__ int hist[2048];
    __shared__ int part[32];
    __shared__ int s_digit, s_below, s_le, s_cnt;
    const int c = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, CS = C + 1;
    const int n = w.hist[(size_t)b * CS + c];
    if (n == 0) return;                                      // n_cand = more = 0 from pc_offsets
    const size_t off = (size_t)b * N + w.seg_off[(size_t)b * CS + c];
    const unsigned long long* seg = w.seg + off;
    int Cn = n;
    bool ties_overflow = false;
    if (n <= NMS_CAP) {
        for (int i = tid; i < n; i += 1024) sbuf[i] = seg[i];
    } else {                                                 // radix select of the best >= NMS_TOPK keys
        unsigned int prefix = 0, pmask = 0;
        int below = 0;
        const int shifts[3] = {21, 10, 0}, widths[3] = {11, 11, 10};
        for (int level = 0; level < 3; ++level) {
            const int shift = shifts[level], nd = 1 << widths[level];
            for (int i = tid; i < 2048; i += 1024) hist[i] = 0;
            __syncthreads();
            for (int i = tid; i < n; i += 1024) {
                const unsigned int k = (unsigned int)(seg[i] >> 32);
                if ((k & pmask) == prefix) atomicAdd(&hist[(k >> shift) & (nd - 1)], 1);
            }
            __syncthreads();
            if (tid < 32) { int s = 0; for (int d = tid * 64; d < tid * 64 + 64; ++d) s += hist[d]; part[tid] = s; }
            __syncthreads();
            if (tid == 0) {                                  // smallest digit d with below + #(digit <= d) >= NMS_TOPK
                int cum = below, q = 0;
                while (q < 31 && cum + part[q] < NMS_TOPK) { cum += part[q]; ++q; }
                int d = q * 64;
                while (d < q * 64 + 63 && cum + hist[d] < NMS_TOPK) { cum += hist[d]; ++d; }
                s_digit = d; s_below = cum; s_le = cum + hist[d];
            }
            __syncthreads();
            prefix |= (unsigned int)s_digit << shift;
            pmask |= (unsigned int)(nd - 1) << shift;
            below = s_below;
            Cn = s_le;
            __syncthreads();
            if (Cn <= NMS_CAP) break;                        // every key <= this (partial) threshold fits
            if (level == 2) ties_overflow = true;            // > NMS_CAP members share one exact score
        }
        if (ties_overflow) {
            if (tid == 0) { w.need[(size_t)b * CS + c] = 1; w.more[(size_t)b * CS + c] = 1; }
            return;                                          // n_cand stays 0: no tile, an empty scan
        }
        if (tid == 0) s_cnt = 0;
        __syncthreads();
        for (int i = tid; i < n; i += 1024) {
            const unsigned long long k = seg[i];
            if (((unsigned int)(k >> 32) & pmask) <= prefix) sbuf[atomicAdd(&s_cnt, 1)] = k;
        }
    }
    __syncthreads();
    int P2 = 64;
    while (P2 < Cn) P2 <<= 1;
    for (int i = Cn + tid; i < P2; i += 1024) sbuf[i] = ~0ull;
    __syncthreads();
    for (int k = 2; k <= P2; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < P2 / 2; t += 1024) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                ce(sbuf[i], sbuf[i + j], (i & k) == 0);
            }
            __syncthreads();
        }
    unsigned long long* cand = w.cand + off;
    for (int i = tid; i < Cn; i += 1024) cand[i] = sbuf[i];
    if (tid == 0) { w.n_cand[(size_t)b * CS + c] = Cn; w.more[(size_t)b * CS + c] = n > Cn ? 1 : 0; }
}

__global__ __launch_bounds__(64) void pc_matrix_kernel(const float* boxes, int64_t N, int D, float thr, int C, int64_t R, PcWs w) {
    const int b = blockIdx.y, CS = C + 1;
    const int* toff = w.tile_off + (size_t)b * CS;
    // the image's tiles are dealt round over a grid that does not grow with the class count: a workgroup without a tile
    // costs a launch slot, and most classes have few
    for (int t = blockIdx.x; t < toff[C]; t += gridDim.x) {
        int lo = 0, hi = C - 1;                              // the class of tile t: the last c with toff[c] <= t
        while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (toff[mid] <= t) lo = mid; else hi = mid - 1; }
        const int c = lo;
        int Kc = w.n_cand[(size_t)b * CS + c];               // 0 where pc_select handed the class over
        if (Kc > NMS_TOPK) Kc = NMS_TOPK;
        const int n = w.hist[(size_t)b * CS + c];
        const int T = ((n < NMS_TOPK ? n : NMS_TOPK) + 63) / 64;     // the tile grid pc_offsets counted for this class
        int rb = 0, lt = t - toff[c];                        // row block rb holds the T - rb tiles w = rb .. T-1
        while (lt >= T - rb) { lt -= T - rb; ++rb; }
        const int wd = rb + lt;
        if (rb * 64 >= Kc) continue;
        matrix_tile(boxes + (size_t)b * N * D, D, thr, w.cand + (size_t)b * N + w.seg_off[(size_t)b * CS + c], Kc, rb, wd,
                    w.mask + ((size_t)b * R + w.row_off[(size_t)b * CS + c]) * NMS_WORDS);
        __syncthreads();                                     // the tile's LDS columns are read out before the next tile's land
    }
}

__global__ __launch_bounds__(256) void pc_scan_kernel(int64_t N, int C, int64_t R, int max_out, PcWs w) {
    const int c = blockIdx.x, b = blockIdx.y, CS = C + 1;
    const size_t bc = (size_t)b * CS + c;
    if (w.hist[bc] == 0) return;                             // cnt = 0 from pc_offsets
    scan_prefix(max_out, w.cand + (size_t)b * N + w.seg_off[bc], w.n_cand[bc], &w.more[bc],
                w.mask + ((size_t)b * R + w.row_off[bc]) * NMS_WORDS, w.kidx + ((size_t)b * C + c) * NMS_MAXK,
                &w.cnt[(size_t)b * C + c], &w.need[bc]);
}

__global__ __launch_bounds__(NMS_THREADS) void pc_general_kernel(const float* boxes, int64_t N, int D, int C, int max_out,
                                                                 float thr, PcWs w) {
    __shared__ WalkLds L;
    const int c = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, CS = C + 1;
    const size_t bc = (size_t)b * CS + c;
    const int n = w.hist[bc];
    if (!w.need[bc] || n == 0) return;
    unsigned long long* keys = w.seg + (size_t)b * N + w.seg_off[bc];
    // bitonic sort of an arbitrary length: every comparison ascending (the first step of a merge mirrors its upper
    // half), so the virtual +inf padding beyond n never moves and pairs that reach into it are skipped
    int P2 = 1;
    while (P2 < n) P2 <<= 1;
    for (int k = 2; k <= P2; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < P2 / 2; t += NMS_THREADS) {
                int i, p;
                if (j == (k >> 1)) { const int blk = t / j, o = t - blk * j; i = blk * k + o; p = blk * k + (k - 1 - o); }
                else { i = ((t & ~(j - 1)) << 1) | (t & (j - 1)); p = i + j; }
                if (p < n) {
                    const unsigned long long a = keys[i], q = keys[p];
                    if (a > q) { keys[i] = q; keys[p] = a; }
                }
            }
            __syncthreads();
        }
    int* kidx = w.kidx + ((size_t)b * C + c) * NMS_MAXK;
    const int nk = greedy_walk(L, boxes + (size_t)b * N * D, D, keys, n, max_out, thr,
                               [&](int pos, int idx) { kidx[pos] = idx; });
    if (tid == 0) w.cnt[(size_t)b * C + c] = nk;
}

// SCORE: the soft-NMS's gather -- column obj_idx of a kept row is its output score kscore[b][c][k] instead of the source row's
template <bool SCORE>
__device__ __forceinline__ void pc_finish_body(const float* boxes, int64_t N, int D, int C, int max_out, const PcWs& w,
                                               float* rows, int32_t* kept, int32_t* count, int obj_idx, const float* kscore) {
    __shared__ int pre[BYOLO_MAX_CLASSES + 1];               // kept before class c
    __shared__ int src[PC_ROWS];                             // source row of each output row of this workgroup, -1 = none
    __shared__ float ksc[SCORE ? PC_ROWS : 1];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int* cnt = w.cnt + (size_t)b * C;
    for (int c = tid; c < C; c += 256) pre[c + 1] = cnt[c];
    __syncthreads();
    if (tid == 0) { int s = 0; for (int c = 0; c < C; ++c) { const int n = pre[c + 1]; pre[c] = s; s += n; } pre[C] = s; }
    __syncthreads();
    const int total = pre[C], cap = C * max_out, k0 = blockIdx.x * PC_ROWS;
    const int nrow = cap - k0 < PC_ROWS ? cap - k0 : PC_ROWS;
    if (tid < nrow) {
        const int k = k0 + tid;
        int idx = -1;
        if (k < total) {
            int lo = 0, hi = C - 1;                          // the last class with pre[c] <= k
            while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (pre[mid] <= k) lo = mid; else hi = mid - 1; }
            idx = w.kidx[((size_t)b * C + lo) * NMS_MAXK + (k - pre[lo])];
            if (SCORE) ksc[tid] = kscore[((size_t)b * C + lo) * NMS_MAXK + (k - pre[lo])];
        }
        src[tid] = idx;
        kept[(size_t)b * cap + k] = idx;
    }
    __syncthreads();
    const float* bx = boxes + (size_t)b * N * D;
    float* ro = rows + ((size_t)b * cap + k0) * D;
    for (int e = tid; e < nrow * D; e += 256) {
        const int k = e / D, col = e - k * D;
        ro[e] = src[k] >= 0 ? ((SCORE && col == obj_idx) ? ksc[k] : bx[(size_t)src[k] * D + col]) : 0.f;
    }
    if (blockIdx.x == 0 && tid == 0) { count[2 * b] = total; count[2 * b + 1] = cnt[0]; }
}
__global__ __launch_bounds__(256) void pc_finish_kernel(const float* boxes, int64_t N, int D, int C, int max_out, PcWs w,
                                                        float* rows, int32_t* kept, int32_t* count) {
    pc_finish_body<false>(boxes, N, D, C, max_out, w, rows, kept, count, -1, nullptr);
}

hipError_t launch_sort_nms(const NmsParams& p, hipStream_t st) {
    const int C = p.C;
    if (p.max_out > NMS_MAXK || p.max_out < 1 || C < 1 || C > BYOLO_MAX_CLASSES) return hipErrorInvalidValue;
    if (C > 1 && (p.cls_start < 0 || p.cls_start + C > p.D)) return hipErrorInvalidValue;
    if (p.N >= (1ll << 31) || p.ws_bytes < pc_ws_layout(p.B, p.N, C, nullptr, nullptr)) return hipErrorInvalidValue;
    PcWs w;
    pc_ws_layout(p.B, p.N, C, reinterpret_cast<char*>(p.ws), &w);
    const int64_t R = pc_mask_rows(p.N, C);
    const dim3 by_row((unsigned)((p.N + 255) / 256), p.B), by_tile((unsigned)((p.N + PC_TILE - 1) / PC_TILE), p.B), by_class(C, p.B);
    // (a kernel, not a memset node: a forward captured as a launch graph replays this sequence -- see launch_zero_words)
    if (hipError_t e = launch_zero_words(w.hist, (int64_t)2 * p.B * (C + 1), st); e != hipSuccess) return e;
    if (C <= PC_DIRECT_C)
        hipLaunchKernelGGL(pc_classify_kernel, by_row, dim3(256), 0, st, p.boxes, p.N, p.D, p.obj_idx, p.cls_start, C, w.cls, w.hist);
    else
        hipLaunchKernelGGL(pc_classify_tiled_kernel, by_tile, dim3(256), 0, st, p.boxes, p.N, p.D, p.obj_idx, p.cls_start, C, w.cls, w.hist);
    hipLaunchKernelGGL(pc_offsets_kernel, dim3(p.B), dim3(64), 0, st, C, p.general_only != 0 ? 1 : 0, w);
    hipLaunchKernelGGL(pc_scatter_kernel, by_row, dim3(256), 0, st, p.boxes, p.N, p.D, p.obj_idx, C, w);
    if (!p.general_only) {
        static std::atomic<uint64_t> sel_attr_done{0}, scan_attr_done{0};
        const size_t lds = (size_t)NMS_CAP * sizeof(unsigned long long);
        if (hipError_t e = set_dynamic_lds_once(reinterpret_cast<const void*>(pc_select_kernel), lds, sel_attr_done); e != hipSuccess) return e;
        const size_t scan_lds = (size_t)2 * 64 * NMS_WORDS * sizeof(unsigned long long);
        if (hipError_t e = set_dynamic_lds_once(reinterpret_cast<const void*>(pc_scan_kernel), scan_lds, scan_attr_done); e != hipSuccess) return e;
        hipLaunchKernelGGL(pc_select_kernel, by_class, dim3(1024), lds, st, p.N, C, w);
        // enough one-wave workgroups to fill the chip's wave slots over the batch, never more than there can be tiles
        const int64_t mgrid = std::min<int64_t>(pc_max_tiles(p.N, C), std::max(512, std::min(8192, 32768 / p.B)));
        hipLaunchKernelGGL(pc_matrix_kernel, dim3((unsigned)mgrid, p.B), dim3(64), 0, st, p.boxes, p.N, p.D,
                           p.iou_thr, C, R, w);
        hipLaunchKernelGGL(pc_scan_kernel, by_class, dim3(256), scan_lds, st, p.N, C, R, p.max_out, w);
    }
    hipLaunchKernelGGL(pc_general_kernel, by_class, dim3(NMS_THREADS), 0, st, p.boxes, p.N, p.D, C, p.max_out, p.iou_thr, w);
    hipLaunchKernelGGL(pc_finish_kernel, dim3((unsigned)(((int64_t)C * p.max_out + PC_ROWS - 1) / PC_ROWS), p.B), dim3(256), 0, st,
                       p.boxes, p.N, p.D, C, p.max_out, w, p.rows, p.kept, p.count);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// Soft-NMS (Bodla et al., ICCV 2017, Algorithm 1; include/byolo.h "soft-NMS"): per (image, class) the candidate with the largest
// CURRENT score is picked, and every remaining candidate's score is multiplied by a weight of its IoU with the pick -- linear
// (1 - v above iou_soft) or Gaussian (exp(-v^2 / sigma), formed in float64, rounded once) -- until max_out rows are picked or no
// candidate's score is above min_score; a candidate also leaves when its IoU with a pick exceeds iou_hard.  The class segments are
// the hard pipeline's (pc_classify / pc_offsets / pc_scatter); then
//   soft_pick     grid (class, image), one 512-thread workgroup: the members with score > min_score are compacted, then the
//                 pick loop.  A pick is one arg-max over the workgroup -- every thread keeps the best (score bits, ~row index) key
//                 of its own candidates up to date while it applies the decay, a wave reduction and 8 LDS words do the rest --
//                 and one broadcast of the picked box through LDS: two barriers.  The key orders equal scores by the lower row
//                 index, so the result does not depend on where the (atomically ordered) compaction put a candidate.
//                   resident path: up to SOFT_NMS_RESIDENT_CAP candidates, 16 per thread in registers (box, area, score, index),
//                                  walked with fully unrolled loops; slots beyond the candidate count are skipped uniformly
//                   general path:  any count (and every class under byolo_plan_opts.nms_general): the current scores live in the
//                                  workspace, boxes are re-read from the rows for every pick -- exact, slow
//                 Both take soft_iou / soft_gauss / soft_apply on the same values in the same order per candidate: the same bytes.
//   soft_finish   pc_finish's gather with the obj_idx column replaced by the output score
// The float64 part is skipped where the IoU is 0 (the weight is exactly 1 there).
// ------------------------------------------------------------------------------------------------
static constexpr int SOFT_THREADS = 512;                      // 8 waves, two per SIMD: 256 registers a lane for the 16 resident slots
static constexpr int SOFT_SLOTS = SOFT_NMS_RESIDENT_CAP / SOFT_THREADS;
static_assert(SOFT_SLOTS * SOFT_THREADS == SOFT_NMS_RESIDENT_CAP, "the resident capacity is whole slots of the workgroup");

struct SoftCfg { int method; float sigma, iou_soft, iou_hard, min_score; };
struct SoftWs {
    PcWs pc;                                                 // mask and cand stay null: the prefix path does not run
    int* cidx;                                               // [B][N] row indices of the candidates (score > min_score), by class segment
    float* cur;                                              // [B][N] current scores of the general path, beside cidx
    float* kscore;                                           // [B][C][NMS_MAXK] output scores, beside pc.kidx
};
static size_t soft_ws_layout(int B, int64_t N, int C, char* base, SoftWs* w) {
    size_t o = 0;
    auto take = [&](size_t bytes) { char* p = base ? base + o : nullptr; o += (bytes + 255) / 256 * 256; return p; };
    const size_t ci = (size_t)B * (C + 1) * 4;
    char* hc = take(2 * ci);                                 // hist + cursor: cleared by one launch_zero_words
    char* so = take(ci); char* ro = take(ci); char* to = take(ci); char* nc = take(ci); char* mo = take(ci); char* ne = take(ci);
    char* cn = take((size_t)B * C * 4);
    char* cl = take((size_t)B * N);
    char* sg = take((size_t)B * N * 8);
    char* ki = take((size_t)B * C * NMS_MAXK * 4); char* ks = take((size_t)B * C * NMS_MAXK * 4);
    char* cx = take((size_t)B * N * 4); char* cu = take((size_t)B * N * 4);
    if (w) { *w = SoftWs{};
             w->pc.hist = (int*)hc; w->pc.cursor = (int*)(hc ? hc + ci : nullptr); w->pc.seg_off = (int*)so; w->pc.row_off = (int*)ro;
             w->pc.tile_off = (int*)to; w->pc.n_cand = (int*)nc; w->pc.more = (int*)mo; w->pc.need = (int*)ne; w->pc.cnt = (int*)cn;
             w->pc.cls = (unsigned char*)cl; w->pc.seg = (unsigned long long*)sg; w->pc.kidx = (int*)ki;
             w->kscore = (float*)ks; w->cidx = (int*)cx; w->cur = (float*)cu; }
    return o;
}
size_t soft_nms_workspace_bytes(int B, int64_t N, int C) { return soft_ws_layout(B, N, C, nullptr, nullptr); }
const int32_t* soft_nms_class_counts_ptr(void* ws, int B, int64_t N, int C) {
    SoftWs w;
    soft_ws_layout(B, N, C, reinterpret_cast<char*>(ws), &w);
    return w.pc.cnt;
}

// What one pick `pk` does to a live candidate `me` of current score s, in three steps that both paths take in this order.  One
// rounding per float32 operation; the Gaussian weight one operation per line in float64, rounded once (plain operators with
// contraction off: see iou_value_rn).
__device__ __forceinline__ float soft_iou(const NBox& pk, const NBox& me) {
    const float v = iou_value_rn(pk, me);
    return (v >= 0.f) ? v : 0.f;                             // a NaN counts as 0
}
__device__ __forceinline__ float soft_linear(float v) {
#pragma clang fp contract(off)
    return 1.f - v;
}
__device__ __forceinline__ float soft_gauss(float v, float sigma) {
#pragma clang fp contract(off)
    const double vv = (double)v * (double)v;
    const double q = vv / (double)sigma;
    return (float)exp(-q);
}
// the new score, 0 = the candidate leaves.  (A live score is > min_score >= 0, so 0 marks the dead.)
__device__ __forceinline__ float soft_apply(float s, float v, float wgt, const SoftCfg& c) {
#pragma clang fp contract(off)
    s = s * wgt;
    return (v > c.iou_hard || !(s > c.min_score)) ? 0.f : s;
}
// arg-max key of a live candidate: larger score first, then the LOWER row index
__device__ __forceinline__ unsigned long long soft_key(float s, int idx) {
    return ((unsigned long long)__float_as_uint(s) << 32) | (0xFFFFFFFFu - (unsigned int)idx);
}
__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long k) {
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned int lo = __shfl_xor((unsigned int)k, o), hi = __shfl_xor((unsigned int)(k >> 32), o);
        const unsigned long long q = ((unsigned long long)hi << 32) | lo;
        k = q > k ? q : k;
    }
    return k;
}
struct SoftLds { unsigned long long wmax[SOFT_THREADS / 64]; float pk[5]; };
// The workgroup's best key from every thread's: 0 = no live candidate (uniform).  One barrier; the caller's second barrier (behind
// the owner's broadcast) also separates this call's reads of wmax from the next call's writes.
__device__ __forceinline__ unsigned long long soft_argmax(SoftLds& L, unsigned long long best) {
    const unsigned long long wb = wave_max_u64(best);
    if ((threadIdx.x & 63) == 0) L.wmax[threadIdx.x >> 6] = wb;
    __syncthreads();
    unsigned long long g = 0ull;
#pragma unroll
    for (int k = 0; k < SOFT_THREADS / 64; ++k) { const unsigned long long q = L.wmax[k]; g = q > g ? q : g; }
    return g;
}

template <class Emit>
__device__ __forceinline__ int soft_walk_resident(SoftLds& L, const float* bx, int D, int obj_idx, const int* cidx, int nc,
                                                  int max_out, const SoftCfg& c, Emit emit) {
    const int tid = threadIdx.x;
    float y0[SOFT_SLOTS], x0[SOFT_SLOTS], y1[SOFT_SLOTS], x1[SOFT_SLOTS], ar[SOFT_SLOTS], sc[SOFT_SLOTS];
    int ix[SOFT_SLOTS];
    const int nslot = (nc + SOFT_THREADS - 1) / SOFT_THREADS;  // slots >= nslot are empty in every thread
    unsigned long long best = 0ull;
    int bs = 0;
#pragma unroll
    for (int s = 0; s < SOFT_SLOTS; ++s) {
        const int i = s * SOFT_THREADS + tid;
        y0[s] = x0[s] = y1[s] = x1[s] = ar[s] = sc[s] = 0.f; ix[s] = 0;
        if (i < nc) {
            const int idx = cidx[i];
            const float* r = bx + (size_t)idx * D;
            const NBox me = make_box(r[0], r[1], r[2], r[3]);
            y0[s] = me.y0; x0[s] = me.x0; y1[s] = me.y1; x1[s] = me.x1; ar[s] = me.area; sc[s] = r[obj_idx]; ix[s] = idx;
            const unsigned long long k = soft_key(sc[s], idx);
            if (k > best) { best = k; bs = s; }
        }
    }
    int nk = 0;
    while (nk < max_out) {
        const unsigned long long g = soft_argmax(L, best);
        if (g == 0ull) break;
        if (best == g) {                                     // the owner: row indices are unique, so exactly one thread
#pragma unroll
            for (int s = 0; s < SOFT_SLOTS; ++s)
                if (s == bs) { L.pk[0] = y0[s]; L.pk[1] = x0[s]; L.pk[2] = y1[s]; L.pk[3] = x1[s]; L.pk[4] = ar[s]; sc[s] = 0.f; }
            emit(nk, (int)(0xFFFFFFFFu - (unsigned int)g), __uint_as_float((unsigned int)(g >> 32)));
        }
        ++nk;
        __syncthreads();
        if (nk >= max_out) break;                            // the last pick decays nobody who could still be picked
        const NBox pk = {L.pk[0], L.pk[1], L.pk[2], L.pk[3], L.pk[4]};
        // the IoU of every live slot; the float64 weights are then formed at ONE place, for the slots that overlap the pick at all
        // (v == 0: the weight is exactly 1) -- sixteen inlined copies of exp() would not fit the register file
        float wv[SOFT_SLOTS];                                // the slot's weight (Gaussian, until its turn below: its IoU)
        unsigned int need = 0u, hard = 0u;
#pragma unroll
        for (int s = 0; s < SOFT_SLOTS; ++s) {
            wv[s] = 1.f;
            if (s < nslot && sc[s] != 0.f) {
                const NBox me = {y0[s], x0[s], y1[s], x1[s], ar[s]};
                const float v = soft_iou(pk, me);
                if (v > c.iou_hard) hard |= 1u << s;
                if (c.method == SOFT_NMS_LINEAR) { if (v > c.iou_soft) wv[s] = soft_linear(v); }
                else if (v != 0.f) { wv[s] = v; need |= 1u << s; }
            }
        }
        while (need) {
            const int s0 = __builtin_ctz(need);
            need &= need - 1u;
            float v = 0.f;
#pragma unroll
            for (int s = 0; s < SOFT_SLOTS; ++s) if (s == s0) v = wv[s];
            const float wgt = soft_gauss(v, c.sigma);
#pragma unroll
            for (int s = 0; s < SOFT_SLOTS; ++s) if (s == s0) wv[s] = wgt;
        }
        best = 0ull; bs = 0;
#pragma unroll
        for (int s = 0; s < SOFT_SLOTS; ++s) {
            if (s < nslot && sc[s] != 0.f) {
                sc[s] = soft_apply(sc[s], ((hard >> s) & 1u) ? 2.f : 0.f, wv[s], c);         // (2 > iou_hard <= 1: the slot's IoU was)
                if (sc[s] != 0.f) {
                    const unsigned long long k = soft_key(sc[s], ix[s]);
                    if (k > best) { best = k; bs = s; }
                }
            }
        }
    }
    return nk;
}

// Any candidate count: candidate i belongs to thread i % 512 for the whole walk, so cur[i] is read and written by one thread alone.
template <class Emit>
__device__ __forceinline__ int soft_walk_general(SoftLds& L, const float* bx, int D, int obj_idx, const int* cidx, float* cur, int nc,
                                                 int max_out, const SoftCfg& c, Emit emit) {
    const int tid = threadIdx.x;
    unsigned long long best = 0ull;
    int bp = 0;
    for (int i = tid; i < nc; i += SOFT_THREADS) {
        const int idx = cidx[i];
        const float s = bx[(size_t)idx * D + obj_idx];
        cur[i] = s;
        const unsigned long long k = soft_key(s, idx);
        if (k > best) { best = k; bp = i; }
    }
    int nk = 0;
    while (nk < max_out) {
        const unsigned long long g = soft_argmax(L, best);
        if (g == 0ull) break;
        if (best == g) {
            const float* r = bx + (size_t)cidx[bp] * D;
            const NBox me = make_box(r[0], r[1], r[2], r[3]);
            L.pk[0] = me.y0; L.pk[1] = me.x0; L.pk[2] = me.y1; L.pk[3] = me.x1; L.pk[4] = me.area;
            cur[bp] = 0.f;
            emit(nk, (int)(0xFFFFFFFFu - (unsigned int)g), __uint_as_float((unsigned int)(g >> 32)));
        }
        ++nk;
        __syncthreads();
        if (nk >= max_out) break;
        const NBox pk = {L.pk[0], L.pk[1], L.pk[2], L.pk[3], L.pk[4]};
        best = 0ull; bp = 0;
        for (int i = tid; i < nc; i += SOFT_THREADS) {
            float s = cur[i];
            if (s == 0.f) continue;
            const int idx = cidx[i];
            const float* r = bx + (size_t)idx * D;
            const float v = soft_iou(pk, make_box(r[0], r[1], r[2], r[3]));
            float wgt = 1.f;
            if (c.method == SOFT_NMS_LINEAR) { if (v > c.iou_soft) wgt = soft_linear(v); }
            else if (v != 0.f) wgt = soft_gauss(v, c.sigma);
            s = soft_apply(s, v, wgt, c);
            cur[i] = s;
            if (s != 0.f) {
                const unsigned long long k = soft_key(s, idx);
                if (k > best) { best = k; bp = i; }
            }
        }
    }
    return nk;
}

__global__ __launch_bounds__(SOFT_THREADS) void soft_pick_kernel(const float* boxes, int64_t N, int D, int obj_idx, int C, int max_out,
                                                                int general_only, SoftCfg c, SoftWs w) {
    __shared__ SoftLds L;
    __shared__ int s_nc;
    const int cl = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, CS = C + 1;
    const size_t bc = (size_t)b * CS + cl;
    const int n = w.pc.hist[bc];
    if (n == 0) return;                                      // cnt = 0 from pc_offsets
    const size_t off = (size_t)b * N + w.pc.seg_off[bc];
    const float* bx = boxes + (size_t)b * N * D;
    const unsigned long long* seg = w.pc.seg + off;
    int* cidx = w.cidx + off;
    if (tid == 0) s_nc = 0;
    __syncthreads();
    for (int i = tid; i < n; i += SOFT_THREADS) {             // the members above min_score, in any order (see soft_key)
        const int idx = (int)(seg[i] & 0xFFFFFFFFull);
        if (bx[(size_t)idx * D + obj_idx] > c.min_score) cidx[atomicAdd(&s_nc, 1)] = idx;
    }
    __syncthreads();
    const int nc = s_nc;
    int* kidx = w.pc.kidx + ((size_t)b * C + cl) * NMS_MAXK;
    float* ksc = w.kscore + ((size_t)b * C + cl) * NMS_MAXK;
    auto emit = [&](int pos, int idx, float score) { kidx[pos] = idx; ksc[pos] = score; };
    int nk;
    if (nc <= SOFT_NMS_RESIDENT_CAP && !general_only) nk = soft_walk_resident(L, bx, D, obj_idx, cidx, nc, max_out, c, emit);
    else nk = soft_walk_general(L, bx, D, obj_idx, cidx, w.cur + off, nc, max_out, c, emit);
    if (tid == 0) w.pc.cnt[(size_t)b * C + cl] = nk;
}

__global__ __launch_bounds__(256) void soft_finish_kernel(const float* boxes, int64_t N, int D, int obj_idx, int C, int max_out, SoftWs w,
                                                          float* rows, int32_t* kept, int32_t* count) {
    pc_finish_body<true>(boxes, N, D, C, max_out, w.pc, rows, kept, count, obj_idx, w.kscore);
}

hipError_t launch_soft_nms(const SoftNmsParams& sp, hipStream_t st) {
    const NmsParams& p = sp.n;
    const int C = p.C;
    if (p.max_out > NMS_MAXK || p.max_out < 1 || C < 1 || C > BYOLO_MAX_CLASSES) return hipErrorInvalidValue;
    if (C > 1 && (p.cls_start < 0 || p.cls_start + C > p.D)) return hipErrorInvalidValue;
    if (p.obj_idx < 0 || p.obj_idx >= p.D) return hipErrorInvalidValue;
    if (p.N >= (1ll << 31) || p.ws_bytes < soft_ws_layout(p.B, p.N, C, nullptr, nullptr)) return hipErrorInvalidValue;
    if (sp.method != SOFT_NMS_LINEAR && sp.method != SOFT_NMS_GAUSSIAN) return hipErrorInvalidValue;
    if (!(sp.min_score >= 0.f)) return hipErrorInvalidValue;  // 0 marks a dead candidate: live scores are above min_score >= 0
    SoftWs w;
    soft_ws_layout(p.B, p.N, C, reinterpret_cast<char*>(p.ws), &w);
    const SoftCfg c = {sp.method, sp.sigma, sp.iou_soft, sp.iou_hard, sp.min_score};
    const dim3 by_row((unsigned)((p.N + 255) / 256), p.B), by_tile((unsigned)((p.N + PC_TILE - 1) / PC_TILE), p.B), by_class(C, p.B);
    if (hipError_t e = launch_zero_words(w.pc.hist, (int64_t)2 * p.B * (C + 1), st); e != hipSuccess) return e;
    if (C <= PC_DIRECT_C)
        hipLaunchKernelGGL(pc_classify_kernel, by_row, dim3(256), 0, st, p.boxes, p.N, p.D, p.obj_idx, p.cls_start, C, w.pc.cls, w.pc.hist);
    else
        hipLaunchKernelGGL(pc_classify_tiled_kernel, by_tile, dim3(256), 0, st, p.boxes, p.N, p.D, p.obj_idx, p.cls_start, C, w.pc.cls, w.pc.hist);
    hipLaunchKernelGGL(pc_offsets_kernel, dim3(p.B), dim3(64), 0, st, C, 0, w.pc);
    hipLaunchKernelGGL(pc_scatter_kernel, by_row, dim3(256), 0, st, p.boxes, p.N, p.D, p.obj_idx, C, w.pc);
    hipLaunchKernelGGL(soft_pick_kernel, by_class, dim3(SOFT_THREADS), 0, st, p.boxes, p.N, p.D, p.obj_idx, C, p.max_out,
                       p.general_only != 0 ? 1 : 0, c, w);
    hipLaunchKernelGGL(soft_finish_kernel, dim3((unsigned)(((int64_t)C * p.max_out + PC_ROWS - 1) / PC_ROWS), p.B), dim3(256), 0, st,
                       p.boxes, p.N, p.D, p.obj_idx, C, p.max_out, w, p.rows, p.kept, p.count);
    return hipGetLastError();
}

}  // namespace byk
