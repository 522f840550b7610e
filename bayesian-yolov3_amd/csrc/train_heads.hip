// train_heads.hip -- one training step of the three detection heads with a frozen Darknet-53 (include/byolo.h byolo_trainer_*)
//
// The reference trains with `'freeze_darknet53': True` only (uncertainty_training.py:30, yolov3_training.py:29,
// pretraining.py:29): Darknet-53 runs in inference mode (lib_yolo/yolov3.py:531-533) and `optimizer.minimize` (lib_yolo/train.py:88)
// reaches the layers after it.  One byolo_trainer_step is one `sess.run([train_step, ...])` (lib_yolo/train.py:53-54, :84-88):
//
//   backbone   byolo_forward's own launches up to byolo_mark_backbone_end, on the bound handle, in its precision (byolo_run_backbone);
//              the tensors the heads read (the taps) are copied out as fp32
//   forward    per head convolution: z = conv(x) (no bias) -> dropout (p of the handle, inverted: z / (1 - p) * keep, only where the
//              layer has it) -> BN with BATCH statistics over B*H*W (biased variance, eps 1e-5) -> leaky ReLU 0.1 (lib_yolo/layers.py:
//              510-574 with training=True); detection conv 1x1 + bias, linear; route / upsample / concat as the graph says
//   loss       byolo_loss per detection layer (+ its gradient), the L2 term over every kernel and detection bias of the handle
//   backward   BN / leaky / dropout backward per convolution, dW = im2col(x)^T dz (wgrad), dx = dz W^T (dgrad: a forward convolution of
//              dz with the kernel rotated by 180 degrees and ci / co swapped); gradients of a tensor read twice add; only the
//              upsampled channels of a concat carry gradient (the backbone's are dropped)
//   update     moving statistics (momentum 0.99: mv -= (mv - batch) * (1 - 0.99); the moving VARIANCE takes the Bessel-corrected
//              batch variance, as TF 1.x's fused batch norm does) and Adam with TF1's formulas over one flat buffer:
//              g += 0.0005 w (L2 tensors), m += (g - m)(1 - b1), v += (g^2 - v)(1 - b2), w -= lr_t m / (sqrt(v) + eps),
//              lr_t = lr sqrt(1 - b2^t) / (1 - b1^t)
//
// Every convolution GEMM runs in exact fp32 on v_mfma_f32_32x32x2_f32 (gemm_f32_kernel): 128 x 128 output tiles, K in steps of 16
// through LDS, 4 waves of 2 x 2 32 x 32 accumulators each.  Gradients are not split-f16: they span far below the window the hi / lo
// encoding holds.  Every reduction runs in a fixed order: the wgrad GEMM over fixed pixel slices into a partial buffer,
// combined slice by slice; per-channel sums in double over a fixed grid.  Two runs on the same inputs give the same bits.
#include "byolo_internal.h"

#include <stdexcept>

namespace {

// ---------------------------------------------------------------------------------------------------------------------
// fp32 matrix-pipe GEMM with convolution index maps
//   mode 0 (forward / dgrad): C[m][n] (+)= sum_k im2col(x)[m][k] * b[k][n] (+ bias[n]);  m = pixel (s, y, x), k = (tap, ci)
//   mode 1 (wgrad):           P[slice][k][n] = sum_{m in slice} im2col(x)[m][k] * b[m][n];  b = dz [pixels][N]
// 3x3 convolutions are stride 1, SAME (pad 1); 1x1 pad 0.  Output spatial size = input spatial size.
// ---------------------------------------------------------------------------------------------------------------------
struct GemmArgs {
    int mode;
    const float* x; int S, H, W, Cin, ks, pad;
    const float* b; int N;
    float* c; int ldc;
    int Mo, Kred;                // rows of C, reduction length
    int kslice; size_t pstride;  // mode 1: reduction rows per slice (multiple of 16), floats between slices
    const float* bias; int accumulate;
};
constexpr int BM = 128, BN = 128, BK = 16, GT = 256;
typedef float f32x16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ void im2col8(const GemmArgs& a, int pix, int k, int kend, float v[8]) {
    // 8 consecutive reduction indices k .. k+7 of pixel `pix` (guards: pix < S*H*W checked by the caller, k < kend)
    const int HW = a.H * a.W;
    const int s = pix / HW, r = pix - s * HW, y = r / a.W, x = r - (r / a.W) * a.W;
    if ((a.Cin & 7) == 0 && k + 8 <= kend) {
        const int tap = k / a.Cin, ci = k - tap * a.Cin;
        const int iy = y + tap / a.ks - a.pad, ix = x + tap % a.ks - a.pad;
        if (iy < 0 || iy >= a.H || ix < 0 || ix >= a.W) { for (int j = 0; j < 8; ++j) v[j] = 0.f; return; }
        const float4* p = reinterpret_cast<const float4*>(a.x + ((size_t)(s * a.H + iy) * a.W + ix) * a.Cin + ci);
        const float4 u0 = p[0], u1 = p[1];
        v[0] = u0.x; v[1] = u0.y; v[2] = u0.z; v[3] = u0.w; v[4] = u1.x; v[5] = u1.y; v[6] = u1.z; v[7] = u1.w;
        return;
    }
    for (int j = 0; j < 8; ++j) {
        const int kk = k + j;
        float t = 0.f;
        if (kk < kend) {
            const int tap = kk / a.Cin, ci = kk - tap * a.Cin;
            const int iy = y + tap / a.ks - a.pad, ix = x + tap % a.ks - a.pad;
            if (iy >= 0 && iy < a.H && ix >= 0 && ix < a.W) t = a.x[((size_t)(s * a.H + iy) * a.W + ix) * a.Cin + ci];
        }
        v[j] = t;
    }
}

// KIND: 0 forward, 1 dgrad (both mode 0), 2 wgrad (mode 1) -- one instantiation per kind, so a kernel trace separates them.
// LDS rows are padded by 4 floats: the transposing A stores of mode 0 (thread pairs 8 rows apart) and the column stores of mode 1
// (16 pixel rows) then fall on different banks; rows stay 16-byte aligned for the vector stores.
constexpr int LPAD = 4;
template <int KIND>
__global__ __launch_bounds__(GT) void gemm_f32_kernel(const GemmArgs a) {
    constexpr int MODE = KIND == 2 ? 1 : 0;
    __shared__ __attribute__((aligned(16))) float As[BK][BM + LPAD];
    __shared__ __attribute__((aligned(16))) float Bs[BK][BN + LPAD];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6, wm = wv >> 1, wn = wv & 1;
    const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;
    const int npix = a.S * a.H * a.W;
    int kbeg = 0, kend = a.Kred;
    if (MODE == 1) { kbeg = blockIdx.z * a.kslice; kend = min(a.Kred, kbeg + a.kslice); }
    f32x16 acc[2][2];
    for (int i = 0; i < 2; ++i) for (int j = 0; j < 2; ++j) for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    for (int k0 = kbeg; k0 < kend; k0 += BK) {
        float v[8];
        if (MODE == 0) {                                          // A tile: pixel row t/2, reduction columns (t&1)*8 .. +8
            const int r = t >> 1, kk = (t & 1) * 8, m = m0 + r;
            if (m < a.Mo) im2col8(a, m, k0 + kk, kend, v); else for (int j = 0; j < 8; ++j) v[j] = 0.f;
            for (int j = 0; j < 8; ++j) As[kk + j][r] = v[j];
        } else {                                                  // A tile: (tap, ci) rows (t>>4)*8 .. +8, pixel column t&15
            const int c = t & 15, r = (t >> 4) * 8, pix = k0 + c;
            if (pix < kend && m0 + r < a.Mo) {
                // the 8 rows are 8 consecutive (tap, ci) of ONE pixel: im2col8 with the roles of pixel and k as in mode 0
                im2col8(a, pix, m0 + r, a.Mo, v);
            } else for (int j = 0; j < 8; ++j) v[j] = 0.f;
            float4* d = reinterpret_cast<float4*>(&As[c][r]);
            d[0] = make_float4(v[0], v[1], v[2], v[3]); d[1] = make_float4(v[4], v[5], v[6], v[7]);
        }
        {                                                         // B tile: row t>>4, columns (t&15)*8 .. +8 of a row-major [*][N]
            const int kk = t >> 4, n = n0 + (t & 15) * 8, krow = k0 + kk;
            const bool live = krow < kend && (MODE == 1 ? krow < npix : true);
            const float* p = a.b + (size_t)krow * a.N + n;
            if (live && (a.N & 7) == 0 && n + 8 <= a.N) {
                const float4 u0 = reinterpret_cast<const float4*>(p)[0], u1 = reinterpret_cast<const float4*>(p)[1];
                v[0] = u0.x; v[1] = u0.y; v[2] = u0.z; v[3] = u0.w; v[4] = u1.x; v[5] = u1.y; v[6] = u1.z; v[7] = u1.w;
            } else for (int j = 0; j < 8; ++j) v[j] = (live && n + j < a.N) ? p[j] : 0.f;
            float4* d = reinterpret_cast<float4*>(&Bs[kk][(t & 15) * 8]);
            d[0] = make_float4(v[0], v[1], v[2], v[3]); d[1] = make_float4(v[4], v[5], v[6], v[7]);
        }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < BK / 2; ++s) {
            const int kr = 2 * s + (lane >> 5);
            float af[2], bf[2];
            for (int i = 0; i < 2; ++i) af[i] = As[kr][wm * 64 + i * 32 + (lane & 31)];
            for (int j = 0; j < 2; ++j) bf[j] = Bs[kr][wn * 64 + j * 32 + (lane & 31)];
            for (int i = 0; i < 2; ++i)
                for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i], bf[j], acc[i][j], 0, 0, 0);
        }
        __syncthreads();
    }
    // C/D map of the 32x32 f32 MFMA: column lane&31, row (r&3) + 8(r>>2) + 4(lane>>5)
    float* out = MODE == 1 ? a.c + (size_t)blockIdx.z * a.pstride : a.c;
    for (int i = 0; i < 2; ++i)
        for (int j = 0; j < 2; ++j) {
            const int n = n0 + wn * 64 + j * 32 + (lane & 31);
            if (n >= a.N) continue;
            const float bv = a.bias ? a.bias[n] : 0.f;
            for (int r = 0; r < 16; ++r) {
                const int m = m0 + wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                if (m >= a.Mo) continue;
                float* o = out + (size_t)m * a.ldc + n;
                const float val = acc[i][j][r] + bv;
                if (a.accumulate) *o += val; else *o = val;
            }
        }
}

// fixed-order combine of the wgrad slices: dst[i] = sum_s part[s * stride + i]
__global__ void combine_slices_kernel(const float* part, int slices, size_t stride, int64_t n, float* dst) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        float s = part[i];
        for (int k = 1; k < slices; ++k) s += part[k * stride + i];
        dst[i] = s;
    }
}

// dgrad weights: wt[(ky, kx)][co][ci] = w[(ks-1-ky, ks-1-kx)][ci][co]  (a 1x1 kernel: the transpose)
__global__ void rotate_kernel(const float* w, float* wt, int ks, int Cin, int Cout) {
    const int64_t n = (int64_t)ks * ks * Cin * Cout;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int ci = (int)(i % Cin); const int64_t r = i / Cin;
        const int co = (int)(r % Cout); const int tap = (int)(r / Cout);
        const int src_tap = ks * ks - 1 - tap;
        wt[i] = w[((int64_t)src_tap * Cin + ci) * Cout + co];
    }
}

// concat of up to two views [S, H>>sh, W>>sh, C] (nearest-neighbour upsampling by 2^sh) into dst [S, H, W, C0 + C1]
struct Gather { const float* src[2]; int C[2]; int sh[2]; int n; };
__global__ void gather_kernel(const Gather g, float* dst, int S, int H, int W) {
    const int Ct = g.C[0] + (g.n > 1 ? g.C[1] : 0);
    const int64_t total = (int64_t)S * H * W * Ct;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        int c = (int)(i % Ct); const int64_t p = i / Ct;
        const int x = (int)(p % W), y = (int)((p / W) % H), s = (int)(p / ((int64_t)W * H));
        const int k = c < g.C[0] ? 0 : 1; if (k) c -= g.C[0];
        const int sh = g.sh[k], h2 = H >> sh, w2 = W >> sh;
        dst[i] = g.src[k][(((int64_t)s * h2 + (y >> sh)) * w2 + (x >> sh)) * g.C[k] + c];
    }
}

// gradient of one view of a concat: dst[s, y', x', c] (+)= sum over the 2^sh x 2^sh pixels it was copied to of dx[..., c_off + c]
__global__ void scatter_kernel(const float* dx, int S, int H, int W, int Ct, int c_off, int C, int sh, float* dst, int accumulate) {
    const int h2 = H >> sh, w2 = W >> sh, f = 1 << sh;
    const int64_t total = (int64_t)S * h2 * w2 * C;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % C); const int64_t p = i / C;
        const int x = (int)(p % w2), y = (int)((p / w2) % h2), s = (int)(p / ((int64_t)w2 * h2));
        float acc = 0.f;
        for (int dy = 0; dy < f; ++dy)
            for (int dxx = 0; dxx < f; ++dxx) acc += dx[(((int64_t)s * H + y * f + dy) * W + x * f + dxx) * Ct + c_off + c];
        dst[i] = accumulate ? dst[i] + acc : acc;
    }
}

__device__ __forceinline__ bool keep_bit(int64_t i, const uint32_t* bits, uint32_t k0, uint32_t k1, uint32_t thr) {
    return bits ? ((bits[i >> 5] >> (i & 31)) & 1u) != 0 : byolo_keep((uint64_t)i, k0, k1, thr);
}

// per-channel sums in double over a fixed grid of row-strided blocks (the channel_stats_partial pattern, conv_kernels.hip)
constexpr int RED_BLOCKS = 128;                 // (the final passes read RED_BLOCKS partials per channel serially: keep it short)
struct DropArgs { int on; float kp; uint32_t k0, k1, thr; const uint32_t* bits; };

// dropout in place (z = z / kp * keep) and the partial sums of z and z^2 per channel
__global__ void drop_stats_partial(float* z, int64_t M, int C, DropArgs d, double* tmp) {
    for (int c = threadIdx.x; c < C; c += blockDim.x) {
        double s = 0.0, q = 0.0;
        for (int64_t m = blockIdx.x; m < M; m += gridDim.x) {
            const int64_t i = m * C + c;
            float v = z[i];
            if (d.on) { v = (v / d.kp) * (keep_bit(i, d.bits, d.k0, d.k1, d.thr) ? 1.f : 0.f); z[i] = v; }
            s += v; q += (double)v * v;
        }
        tmp[((size_t)blockIdx.x * 2) * C + c] = s;
        tmp[((size_t)blockIdx.x * 2 + 1) * C + c] = q;
    }
}
// mean, biased variance (BN) and the Bessel-corrected variance (moving statistics)
__global__ void stats_final(const double* tmp, int blocks, int64_t M, int C, float* mean, float* var, float* var_u) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    double s = 0.0, q = 0.0;
    for (int b = 0; b < blocks; ++b) { s += tmp[((size_t)b * 2) * C + c]; q += tmp[((size_t)b * 2 + 1) * C + c]; }
    const double mu = s / (double)M;
    double v = q / (double)M - mu * mu;
    if (v < 0) v = 0;
    mean[c] = (float)mu; var[c] = (float)v;
    var_u[c] = (float)(M > 1 ? v * (double)M / (double)(M - 1) : v);
}

__device__ __forceinline__ float bn_rstd(float var) { return 1.f / sqrtf(var + 1e-5f); }

// a = leaky(gamma * (z - mean) * rstd + beta)
__global__ void bn_apply_kernel(const float* z, float* a, int64_t total, int C, const float* mean, const float* var,
                                const float* gamma, const float* beta) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % C);
        const float y = gamma[c] * ((z[i] - mean[c]) * bn_rstd(var[c])) + beta[c];
        a[i] = fmaxf(y, 0.1f * y);
    }
}

// backward, pass 1: per channel sum(dy) and sum(dy * xhat), dy = da * leaky'(y)
__global__ void bn_bwd_partial(const float* da, const float* z, int64_t M, int C, const float* mean, const float* var,
                               const float* gamma, const float* beta, double* tmp) {
    for (int c = threadIdx.x; c < C; c += blockDim.x) {
        const float mu = mean[c], rs = bn_rstd(var[c]), g = gamma[c], b = beta[c];
        double s = 0.0, q = 0.0;
        for (int64_t m = blockIdx.x; m < M; m += gridDim.x) {
            const int64_t i = m * C + c;
            const float xh = (z[i] - mu) * rs, y = g * xh + b;
            const float dy = y > 0.f ? da[i] : 0.1f * da[i];
            s += dy; q += (double)dy * xh;
        }
        tmp[((size_t)blockIdx.x * 2) * C + c] = s;
        tmp[((size_t)blockIdx.x * 2 + 1) * C + c] = q;
    }
}
// dbeta = sum dy, dgamma = sum dy * xhat; k1 = dbeta / M, k2 = dgamma / M for pass 2
__global__ void bn_bwd_final(const double* tmp, int blocks, int64_t M, int C, float* dgamma, float* dbeta, float* k12) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    double s = 0.0, q = 0.0;
    for (int b = 0; b < blocks; ++b) { s += tmp[((size_t)b * 2) * C + c]; q += tmp[((size_t)b * 2 + 1) * C + c]; }
    if (dbeta) dbeta[c] = (float)s;
    if (dgamma) dgamma[c] = (float)q;
    if (k12) { k12[c] = (float)(s / (double)M); k12[C + c] = (float)(q / (double)M); }
}
// backward, pass 2 (in place on da): dz = (gamma * rstd * (dy - dbeta/M - xhat * dgamma/M)) / kp * keep
__global__ void bn_bwd_apply(float* da, const float* z, int64_t total, int C, const float* mean, const float* var,
                             const float* gamma, const float* beta, const float* k12, DropArgs d) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % C);
        const float rs = bn_rstd(var[c]), g = gamma[c];
        const float xh = (z[i] - mean[c]) * rs, y = g * xh + beta[c];
        const float dy = y > 0.f ? da[i] : 0.1f * da[i];
        float dz = (g * rs) * (dy - k12[c] - xh * k12[C + c]);
        if (d.on) dz = (dz / d.kp) * (keep_bit(i, d.bits, d.k0, d.k1, d.thr) ? 1.f : 0.f);
        da[i] = dz;
    }
}

// sum of squares of the L2 part of the flat parameter buffer (partials in double)
__global__ void sumsq_partial(const float* w, int64_t n, double* tmp) {
    __shared__ double red[4];
    double s = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) s += (double)w[i] * w[i];
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) tmp[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}
// losses[6] = total, detection, regularization, loc, obj, cls (lib_yolo/train.py:53-55)
__global__ void losses_kernel(const double* det /*[n_det][3]*/, int n_det, const double* sq, int blocks, double reg_const, double l2,
                              double* out) {
    if (threadIdx.x != 0) return;
    double loc = 0, obj = 0, cls = 0, s = 0;
    for (int k = 0; k < n_det; ++k) { loc += det[3 * k]; obj += det[3 * k + 1]; cls += det[3 * k + 2]; }
    for (int b = 0; b < blocks; ++b) s += sq[b];
    const double reg = reg_const + l2 * s / 2.0, d = loc + obj + cls;
    out[0] = d + reg; out[1] = d; out[2] = reg; out[3] = loc; out[4] = obj; out[5] = cls;
}

// the optimizer: L2 gradient on the first n_l2 elements, then (update) Adam with TF1's ApplyAdam arithmetic
// (c1 = 1 - b1, c2 = 1 - b2: formed in double, then rounded once -- 1 - 0.999f in float32 is 4.7e-5 off 0.001)
__global__ void adam_kernel(float* w, float* g, float* m, float* v, int64_t n, int64_t n_l2, float l2, int update, float lr_t,
                            float c1, float c2, float eps) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const float wi = w[i];
        float gi = g[i];
        if (i < n_l2) gi = gi + l2 * wi;
        g[i] = gi;
        if (!update) continue;
        float mi = m[i], vi = v[i];
        mi = mi + (gi - mi) * c1;
        vi = vi + (gi * gi - vi) * c2;
        m[i] = mi; v[i] = vi;
        w[i] = wi - (lr_t * mi) / (sqrtf(vi) + eps);
    }
}
// moving statistics: mov = [means | variances], batch = [means | Bessel-corrected variances]
__global__ void moving_kernel(float* mov, const float* batch, int64_t n, float decay) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        mov[i] = mov[i] - (mov[i] - batch[i]) * decay;
}

// per-column sums of x [M, C] (the detection bias gradient): reuses the BN partial layout with a zero second row
__global__ void colsum_partial(const float* x, int64_t M, int C, double* tmp) {
    for (int c = threadIdx.x; c < C; c += blockDim.x) {
        double s = 0.0;
        for (int64_t m = blockIdx.x; m < M; m += gridDim.x) s += x[m * C + c];
        tmp[((size_t)blockIdx.x * 2) * C + c] = s;
        tmp[((size_t)blockIdx.x * 2 + 1) * C + c] = 0.0;
    }
}

inline unsigned grid1d(int64_t n) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, 4096)); }

}  // namespace

// =====================================================================================================================
// the trainer object
// =====================================================================================================================
namespace {
struct TVar { std::string name; std::vector<int64_t> shape; size_t off = 0; int64_t n = 0; int hparam = -1; };
struct Part { int tensor; int C; int sh; };                 // a view of a trainer tensor: C channels, upsampled by 2^sh
struct TTensor { int layer; int H, W, C; bool frozen; size_t act = 0, grad = 0; bool grad_set = false; };
struct TConv {
    int layer; bool det; int ks, Cin, Cout, drop_ordinal;
    std::vector<Part> in;        // the input view (one plain part: read in place; otherwise gathered into xbuf)
    int out;                     // trainer tensor of the output (activation / raw)
    int v_kernel = -1, v_gamma = -1, v_beta = -1, v_bias = -1;  // TVar indices
    size_t mov_off = 0;          // channel offset of this layer in the moving / batch statistics arrays
    // per-B workspace offsets (bytes)
    size_t z = 0, xbuf = 0, dx = 0;
    bool in_grad = false;        // some part of the input carries gradient
    int kslice = 0, slices = 0;
};
}  // namespace

struct byolo_trainer {
    byolo_t* h = nullptr;
    byolo_t* fallback = nullptr;
    int device = 0;
    bool on_device = false;                                  // device buffers exist (trainer_device)
    std::vector<float> h_w, h_mov;                           // staged copies until then
    int aleatoric_loss = 0;
    std::vector<TVar> vars;
    std::map<std::string, int> vindex;
    std::vector<TConv> convs;
    std::vector<TTensor> tens;
    std::vector<int> taps;                                   // trainer tensors fed by the backbone
    std::vector<int> det_convs;                              // convs[] index of each detection layer, in order
    int64_t n_flat = 0, n_l2 = 0, n_mov = 0;                // floats
    float *d_w = nullptr, *d_g = nullptr, *d_m = nullptr, *d_v = nullptr, *d_mov = nullptr, *d_wt = nullptr;
    int64_t n_wt = 0;                                        // rotated-kernel scratch (largest kernel)
    double reg_const = 0.0;                                  // L2 of the frozen kernels (a constant)
    int64_t step = 0;
    // layout of the last workspace plan
    int ws_B = -1; size_t ws_total = 0, ws_bb = 0, ws_partial = 0, ws_tmp = 0, ws_k12 = 0, ws_bstat = 0, ws_loss = 0, ws_lossws = 0, ws_sq = 0;
    size_t ws_graw = 0;
    void* last_ws = nullptr;
};

static constexpr double ADAM_B1 = 0.9, ADAM_B2 = 0.999;
static constexpr float L2_SCALE = 0.0005f, ADAM_EPS = 1e-8f, BN_DECAY = (float)(1.0 - 0.99);

static int32_t tfail(byolo_trainer_t* tr, int32_t code, const char* msg) { return fail(tr ? tr->h : nullptr, code, "%s", msg); }

static int32_t trainer_build(byolo_trainer_t* tr) {
    byolo_t* h = tr->h;
    const int nl = (int)h->layers.size(), be = h->backbone_end;
    std::vector<std::vector<Part>> view(nl);                 // per head layer: its output as parts
    std::map<int, int> tap_of;                               // backbone layer -> trainer tensor
    auto tensor_of_src = [&](int r) -> std::vector<Part> {
        if (r >= be) return view[r];
        auto it = tap_of.find(r);
        if (it == tap_of.end()) {
            const Layer& l = h->layers[r];
            if (!l.materialized) throw std::runtime_error("a head reads backbone layer " + std::to_string(r) + ", which has no tensor of its own");
            TTensor t; t.layer = r; t.H = l.H; t.W = l.W; t.C = l.C; t.frozen = true;
            tr->tens.push_back(t); tr->taps.push_back((int)tr->tens.size() - 1);
            it = tap_of.emplace(r, (int)tr->tens.size() - 1).first;
        }
        return {Part{it->second, h->layers[r].C, 0}};
    };
    auto add_var = [&](int pi) {
        const Param& p = h->params[pi];
        TVar v; v.name = p.name; v.shape = p.shape; v.n = p.count(); v.hparam = pi;
        tr->vars.push_back(v); tr->vindex[p.name] = (int)tr->vars.size() - 1;
        return (int)tr->vars.size() - 1;
    };
    for (int i = be; i < nl; ++i) {
        const Layer& l = h->layers[i];
        const int prev = l.prev;
        switch (l.op) {
        case OP_CONV: case OP_DETECTION: {
            if (l.stride != 1 || (l.ksize != 1 && l.ksize != 3)) throw std::runtime_error("head layer '" + l.scope + "': only stride-1 1x1 / 3x3 convolutions train");
            if (l.stacked) throw std::runtime_error("head layer '" + l.scope + "' is T-stacked: build the model with inference_mode=False");
            TConv c; c.layer = i; c.det = l.op == OP_DETECTION; c.ks = l.ksize; c.Cout = l.filters; c.drop_ordinal = l.drop_ordinal;
            c.in = tensor_of_src(prev);
            c.Cin = 0; for (auto& p : c.in) c.Cin += p.C;
            if (c.Cin != l.Cin) throw std::runtime_error("head layer '" + l.scope + "': input channels do not add up");
            for (auto& p : c.in) if (!tr->tens[p.tensor].frozen) c.in_grad = true;
            c.v_kernel = add_var(l.p_kernel);
            if (c.det) c.v_bias = add_var(l.p_bias);
            else {
                if (l.p_gamma < 0 || !(l.norm & BYOLO_NORM_BN)) throw std::runtime_error("head layer '" + l.scope + "' has no batch norm");
                c.v_gamma = add_var(l.p_gamma); c.v_beta = add_var(l.p_beta);
                c.mov_off = (size_t)tr->n_mov; tr->n_mov += l.filters;
            }
            TTensor t; t.layer = i; t.H = l.H; t.W = l.W; t.C = l.filters; t.frozen = false;
            tr->tens.push_back(t); c.out = (int)tr->tens.size() - 1;
            view[i] = {Part{c.out, l.filters, 0}};
            if (c.det) tr->det_convs.push_back((int)tr->convs.size());
            tr->convs.push_back(c);
            break;
        }
        case OP_ROUTE: {
            std::vector<Part> v;
            for (int k = 0; k < l.nref; ++k) { auto p = tensor_of_src(l.ref[k]); v.insert(v.end(), p.begin(), p.end()); }
            view[i] = v; break;
        }
        case OP_UPSAMPLE: {
            auto v = tensor_of_src(prev);
            for (auto& p : v) p.sh += 1;
            view[i] = v; break;
        }
        default:                                             // (a residual or a stack has no scope: the layer's index names it)
            throw std::runtime_error("head layer " + std::to_string(i) + ": only convolution, route, upsample and detection layers train");
        }
    }
    if (tr->det_convs.empty()) throw std::runtime_error("the graph has no detection layer after byolo_mark_backbone_end");
    // flat buffer: L2 tensors (kernels, detection biases) first, then gamma / beta; every segment 64-float aligned
    int64_t off = 0;
    for (int pass = 0; pass < 2; ++pass) {
        for (auto& v : tr->vars) {
            const bool l2 = v.name.size() >= 7 && (v.name.compare(v.name.size() - 7, 7, "/kernel") == 0 || v.name.compare(v.name.size() - 5, 5, "/bias") == 0);
            if (l2 != (pass == 0)) continue;
            v.off = (size_t)off; off += (v.n + 63) / 64 * 64;
        }
        if (pass == 0) tr->n_l2 = off;
    }
    tr->n_flat = off;
    for (auto& c : tr->convs) tr->n_wt = std::max<int64_t>(tr->n_wt, tr->vars[c.v_kernel].n);
    // the L2 of every kernel / bias the trainer does not hold (lib_yolo Model.regularization_loss sums all of them)
    for (const auto& p : h->params) {
        const bool l2 = p.name.size() >= 7 && (p.name.compare(p.name.size() - 7, 7, "/kernel") == 0 || p.name.compare(p.name.size() - 5, 5, "/bias") == 0);
        if (!l2 || tr->vindex.count(p.name)) continue;
        double s = 0; for (float x : p.data) s += (double)x * x;
        tr->reg_const += (double)L2_SCALE * s / 2.0;
    }
    return BYOLO_OK;
}

// the handle's head variables and moving statistics, copied on the host when the trainer is made
static void trainer_stage(byolo_trainer_t* tr) {
    byolo_t* h = tr->h;
    tr->h_w.assign((size_t)tr->n_flat, 0.f); tr->h_mov.assign((size_t)tr->n_mov * 2, 0.f);
    for (auto& v : tr->vars) memcpy(tr->h_w.data() + v.off, h->params[v.hparam].data.data(), sizeof(float) * v.n);
    for (auto& c : tr->convs) {
        if (c.det) continue;
        const Layer& l = h->layers[c.layer];
        memcpy(tr->h_mov.data() + c.mov_off, h->params[l.p_mean].data.data(), sizeof(float) * c.Cout);
        memcpy(tr->h_mov.data() + tr->n_mov + c.mov_off, h->params[l.p_var].data.data(), sizeof(float) * c.Cout);
    }
}

// device state, allocated and filled from the staged copy at the first call that needs it (byolo_trainer_create is host-only)
static int32_t trainer_device(byolo_trainer_t* tr) {
    if (tr->on_device) return BYOLO_OK;
    byolo_t* h = tr->h;
    const std::vector<float>& w = tr->h_w; const std::vector<float>& mov = tr->h_mov;
    HIPCHK(h, hipSetDevice(tr->device));
    const size_t fb = sizeof(float) * (size_t)tr->n_flat;
    HIPCHK(h, hipMalloc(&tr->d_w, fb)); HIPCHK(h, hipMalloc(&tr->d_g, fb)); HIPCHK(h, hipMalloc(&tr->d_m, fb)); HIPCHK(h, hipMalloc(&tr->d_v, fb));
    HIPCHK(h, hipMalloc(&tr->d_mov, sizeof(float) * std::max<int64_t>(1, 2 * tr->n_mov)));
    HIPCHK(h, hipMalloc(&tr->d_wt, sizeof(float) * (size_t)tr->n_wt));
    HIPCHK(h, hipMemcpy(tr->d_w, w.data(), fb, hipMemcpyHostToDevice));
    HIPCHK(h, hipMemset(tr->d_g, 0, fb)); HIPCHK(h, hipMemset(tr->d_m, 0, fb)); HIPCHK(h, hipMemset(tr->d_v, 0, fb));
    if (tr->n_mov) HIPCHK(h, hipMemcpy(tr->d_mov, mov.data(), sizeof(float) * 2 * tr->n_mov, hipMemcpyHostToDevice));
    tr->on_device = true;
    std::vector<float>().swap(tr->h_w); std::vector<float>().swap(tr->h_mov);
    return BYOLO_OK;
}

static void trainer_free(byolo_trainer_t* tr) {
    for (float* p : {tr->d_w, tr->d_g, tr->d_m, tr->d_v, tr->d_mov, tr->d_wt}) if (p) (void)hipFree(p);
}

// per-B workspace layout: [backbone forward | tensors (activation, gradient) | per conv z, gathered input, dgrad output, batch stats |
// wgrad slices | reduction scratch | loss buffers]
static int32_t trainer_plan(byolo_trainer_t* tr, int B) {
    byolo_t* h = tr->h;
    make_plan(h, B, 1);
    size_t off = align_up(h->plan.total, 256);
    tr->ws_bb = h->plan.total;
    auto take = [&](size_t bytes) { const size_t o = off; off = align_up(off + bytes, 256); return o; };
    for (auto& t : tr->tens) {
        const size_t n = (size_t)B * t.H * t.W * t.C * 4;
        t.act = take(n);
        t.grad = t.frozen ? 0 : take(n);
    }
    size_t partial = 0, tmp = (size_t)RED_BLOCKS * 2 * 4;
    for (auto& c : tr->convs) {
        const Layer& l = h->layers[c.layer];
        const int64_t M = (int64_t)B * l.H * l.W;
        c.z = c.det ? 0 : take((size_t)M * c.Cout * 4);
        const bool plain = c.in.size() == 1 && c.in[0].sh == 0;
        c.xbuf = plain ? 0 : take((size_t)M * c.Cin * 4);
        c.dx = (c.in_grad && !plain) ? take((size_t)M * c.Cin * 4) : 0;
        // wgrad: fixed pixel slices, enough blocks to fill the chip, the partial buffer below 256 MB
        const int64_t Kc = (int64_t)c.ks * c.ks * c.Cin;
        const int64_t tiles = ((Kc + BM - 1) / BM) * ((c.Cout + BN - 1) / BN);
        int64_t slices = std::max<int64_t>(1, std::min<int64_t>((1024 + tiles - 1) / tiles, (M + 255) / 256));
        while (slices > 1 && slices * Kc * c.Cout * 4 > ((int64_t)256 << 20)) --slices;
        int64_t ksl = ((M + slices - 1) / slices + BK - 1) / BK * BK;
        c.kslice = (int)ksl; c.slices = (int)((M + ksl - 1) / ksl);
        partial = std::max(partial, (size_t)c.slices * Kc * c.Cout * 4);
        tmp = std::max(tmp, (size_t)RED_BLOCKS * 2 * std::max(c.Cout, 1) * sizeof(double));
    }
    tr->ws_partial = take(partial);
    tr->ws_tmp = take(tmp);
    int maxC = 1; for (auto& c : tr->convs) maxC = std::max(maxC, c.Cout);
    tr->ws_k12 = take((size_t)2 * maxC * 4);
    tr->ws_bstat = take((size_t)3 * std::max<int64_t>(1, tr->n_mov) * 4);   // [mean | var_u | var] per head BN channel
    tr->ws_loss = take(sizeof(double) * 3 * tr->det_convs.size());
    tr->ws_lossws = take(byolo_loss_workspace_bytes());
    tr->ws_sq = take(sizeof(double) * RED_BLOCKS);
    tr->ws_total = off;
    tr->ws_B = B;
    return BYOLO_OK;
}

extern "C" int32_t byolo_trainer_create(byolo_t* h, int32_t aleatoric_loss, byolo_trainer_t** out) {
    if (!h || !out) return fail(h, BYOLO_ERR_ARG, "byolo_trainer_create: null argument");
    *out = nullptr;
    if (h->backbone_end < 0) return fail(h, BYOLO_ERR_STATE, "byolo_trainer_create: the graph has no byolo_mark_backbone_end");
    auto* tr = new (std::nothrow) byolo_trainer();
    if (!tr) return fail(h, BYOLO_ERR_NOMEM, "byolo_trainer_create: out of host memory");
    tr->h = h; tr->device = h->device; tr->aleatoric_loss = aleatoric_loss ? 1 : 0;
    int32_t rc = guarded(h, "byolo_trainer_create", [&] {
        if (!h->lowered) { int32_t r = lower(h); if (r) return r; }
        int32_t r = trainer_build(tr); if (r) return r;
        trainer_stage(tr);
        return (int32_t)BYOLO_OK;
    });
    if (rc) { trainer_free(tr); delete tr; return rc; }
    *out = tr;
    return BYOLO_OK;
}

extern "C" int32_t byolo_trainer_destroy(byolo_trainer_t* tr) {
    if (!tr) return BYOLO_OK;
    if (tr->on_device) {                                     // (the bound handle is not touched: it may be gone already)
        (void)hipSetDevice(tr->device);
        (void)hipDeviceSynchronize();
        trainer_free(tr);
    }
    delete tr;
    return BYOLO_OK;
}

extern "C" int32_t byolo_trainer_set_fallback(byolo_trainer_t* tr, byolo_t* h32) {
    if (!tr) return fail(nullptr, BYOLO_ERR_ARG, "byolo_trainer_set_fallback: null trainer");
    if (h32 && (!h32->finalized || h32->layers.size() != tr->h->layers.size() || h32->backbone_end != tr->h->backbone_end || h32->precision != 0))
        return fail(tr->h, BYOLO_ERR_ARG, "byolo_trainer_set_fallback: not a finalized fp32 handle of the same graph");
    tr->fallback = h32;
    return BYOLO_OK;
}

extern "C" int32_t byolo_trainer_workspace_bytes(byolo_trainer_t* tr, int32_t B, size_t* bytes) {
    if (!tr || !bytes || B < 1) return fail(tr ? tr->h : nullptr, BYOLO_ERR_ARG, "byolo_trainer_workspace_bytes: bad argument");
    return guarded(tr->h, "byolo_trainer_workspace_bytes", [&] {
        int32_t rc = check_run(tr->h, B, 1, "byolo_trainer_workspace_bytes", false); if (rc) return rc;
        rc = trainer_plan(tr, B); if (rc) return rc;
        size_t need = tr->ws_total;
        if (tr->fallback) {                                   // the fp32 backbone's arena lies behind the trainer's buffers
            make_plan(tr->fallback, B, 1);
            need = align_up(tr->ws_total, 256) + tr->fallback->plan.total;
            (void)trainer_plan(tr, B);                        // (the bound handle's plan again)
        }
        *bytes = need;
        return (int32_t)BYOLO_OK;
    });
}

static GemmArgs conv_args(const float* x, int S, int H, int W, int Cin, int ks, const float* b, int N, float* c) {
    GemmArgs a; memset(&a, 0, sizeof a);
    a.mode = 0; a.x = x; a.S = S; a.H = H; a.W = W; a.Cin = Cin; a.ks = ks; a.pad = ks == 3 ? 1 : 0;
    a.b = b; a.N = N; a.c = c; a.ldc = N; a.Mo = S * H * W; a.Kred = ks * ks * Cin;
    return a;
}
enum { GEMM_FWD = 0, GEMM_DGRAD = 1, GEMM_WGRAD = 2 };
static hipError_t launch_gemm(const GemmArgs& a, int slices, int kind, hipStream_t st) {
    const dim3 grid((unsigned)((a.Mo + BM - 1) / BM), (unsigned)((a.N + BN - 1) / BN), (unsigned)std::max(1, slices));
    if (kind == GEMM_WGRAD) hipLaunchKernelGGL(gemm_f32_kernel<GEMM_WGRAD>, grid, dim3(GT), 0, st, a);
    else if (kind == GEMM_DGRAD) hipLaunchKernelGGL(gemm_f32_kernel<GEMM_DGRAD>, grid, dim3(GT), 0, st, a);
    else hipLaunchKernelGGL(gemm_f32_kernel<GEMM_FWD>, grid, dim3(GT), 0, st, a);
    return hipGetLastError();
}

static int32_t trainer_step_impl(byolo_trainer_t* tr, const float* d_img, int32_t B, uint64_t seed, const uint32_t* d_mask_bits,
                                 const float* d_gt_loc, const float* d_gt_obj, const int32_t* d_gt_cls, const float* d_gt_ign, float lr,
                                 int32_t grads_only, double* d_losses, void* d_workspace, size_t workspace_bytes, void* stream) {
    byolo_t* h = tr->h;
    if (!d_img || !d_workspace || !d_gt_loc || !d_gt_obj || !d_gt_cls || !d_gt_ign || !d_losses || B < 1)
        return fail(h, BYOLO_ERR_ARG, "byolo_trainer_step: null argument or B < 1");
    int32_t rc = check_run(h, B, 1, "byolo_trainer_step"); if (rc) return rc;
    rc = trainer_device(tr); if (rc) return rc;
    size_t need = 0;
    rc = byolo_trainer_workspace_bytes(tr, B, &need); if (rc) return rc;
    if (workspace_bytes < need) return fail(h, BYOLO_ERR_NOMEM, "byolo_trainer_step: workspace %zu < required %zu bytes", workspace_bytes, need);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    char* ws = reinterpret_cast<char*>(d_workspace);
    auto F = [&](size_t o) { return reinterpret_cast<float*>(ws + o); };
    // ---- backbone (the bound handle; its fp32 twin when an activation leaves the split-f16 range) ----------------------
    byolo_t* bb = h;
    rc = byolo_run_backbone(h, d_img, B, d_workspace, tr->ws_bb, st);
    if (rc == BYOLO_ERR_RANGE && tr->fallback) {
        bb = tr->fallback;
        // the fp32 arena may be larger than the bound handle's: it is laid behind the trainer's own buffers
        make_plan(bb, B, 1);
        const size_t at = align_up(tr->ws_total, 256);
        rc = byolo_run_backbone(bb, d_img, B, ws + at, workspace_bytes - at, st);
        if (rc) return fail(h, rc, "byolo_trainer_step: fp32 backbone: %s", bb->err.c_str());
        for (int ti : tr->taps) {
            const TTensor& t = tr->tens[ti];
            HIPCHK(h, hipMemcpyAsync(F(t.act), ws + at + bb->plan.off[t.layer], (size_t)B * t.H * t.W * t.C * 4, hipMemcpyDeviceToDevice, st));
        }
        rc = trainer_plan(tr, B); if (rc) return rc;          // (make_plan of the bound handle again)
    } else {
        if (rc) return rc;
        for (int ti : tr->taps) {
            const TTensor& t = tr->tens[ti];
            const float* src = reinterpret_cast<const float*>(ws + h->plan.off[t.layer]);
            const int64_t n = (int64_t)B * t.H * t.W * t.C;
            if (h->precision == 1) HIPCHK(h, launch_split_to_f32(src, F(t.act), n, 1.f / ACT_SCALE, st));
            else HIPCHK(h, hipMemcpyAsync(F(t.act), src, (size_t)n * 4, hipMemcpyDeviceToDevice, st));
        }
    }
    tr->last_ws = d_workspace;
    // ---- dropout keys of this step: (seed, step) -> the library's counter stream ----------------------------------------
    const uint64_t sk = seed + (uint64_t)tr->step * 0x9E3779B97F4A7C15ull;
    const float kp = 1.f - h->cfg.drop_prob;
    auto drop_of = [&](const TConv& c) {
        DropArgs d; memset(&d, 0, sizeof d);
        if (c.drop_ordinal < 0) return d;
        if (!d_mask_bits && byolo_drop_is_identity((double)h->cfg.drop_prob)) return d;
        const byolo_drop_keys k = byolo_layer_keys(sk, (uint32_t)c.drop_ordinal, (double)h->cfg.drop_prob);
        d.on = 1; d.kp = kp; d.k0 = k.k0; d.k1 = k.k1; d.thr = k.thr;
        if (d_mask_bits) { int64_t bit = 0; (void)byolo_mask_layout(h, B, 1, c.drop_ordinal, &bit, nullptr); d.bits = d_mask_bits + bit / 32; }
        return d;
    };
    auto input_ptr = [&](const TConv& c) -> const float* {
        return c.xbuf ? F(c.xbuf) : F(tr->tens[c.in[0].tensor].act);
    };
    double* tmp = reinterpret_cast<double*>(ws + tr->ws_tmp);
    float* bmean = F(tr->ws_bstat); float* bvaru = bmean + tr->n_mov; float* bvar = bvaru + tr->n_mov;
    // ---- forward ----------------------------------------------------------------------------------------------------
    for (auto& c : tr->convs) {
        const Layer& l = h->layers[c.layer];
        const int64_t M = (int64_t)B * l.H * l.W;
        if (c.xbuf) {
            Gather g; memset(&g, 0, sizeof g); g.n = (int)c.in.size();
            if (g.n > 2) return fail(h, BYOLO_ERR_ARG, "byolo_trainer_step: a concat of more than two views");
            for (int k = 0; k < g.n; ++k) { g.src[k] = F(tr->tens[c.in[k].tensor].act); g.C[k] = c.in[k].C; g.sh[k] = c.in[k].sh; }
            hipLaunchKernelGGL(gather_kernel, dim3(grid1d(M * c.Cin)), dim3(256), 0, st, g, F(c.xbuf), B, l.H, l.W);
        }
        const float* w = tr->d_w + tr->vars[c.v_kernel].off;
        float* out = c.det ? F(tr->tens[c.out].act) : F(c.z);
        GemmArgs a = conv_args(input_ptr(c), B, l.H, l.W, c.Cin, c.ks, w, c.Cout, out);
        if (c.det) a.bias = tr->d_w + tr->vars[c.v_bias].off;
        HIPCHK(h, launch_gemm(a, 1, GEMM_FWD, st));
        if (c.det) continue;
        const DropArgs d = drop_of(c);
        hipLaunchKernelGGL(drop_stats_partial, dim3(RED_BLOCKS), dim3(256), 0, st, F(c.z), M, c.Cout, d, tmp);
        hipLaunchKernelGGL(stats_final, dim3((c.Cout + 255) / 256), dim3(256), 0, st, tmp, RED_BLOCKS, M, c.Cout,
                           bmean + c.mov_off, bvar + c.mov_off, bvaru + c.mov_off);
        hipLaunchKernelGGL(bn_apply_kernel, dim3(grid1d(M * c.Cout)), dim3(256), 0, st, F(c.z), F(tr->tens[c.out].act), M * c.Cout, c.Cout,
                           bmean + c.mov_off, bvar + c.mov_off, tr->d_w + tr->vars[c.v_gamma].off, tr->d_w + tr->vars[c.v_beta].off);
        HIPCHK(h, hipGetLastError());
    }
    // ---- loss of every detection layer (+ d loss / d raw into the raw output's gradient buffer) ---------------------------
    int64_t N_all = 0;
    for (int ci : tr->det_convs) { const Layer& l = h->layers[tr->convs[ci].layer]; N_all += (int64_t)l.H * l.W * 3; }
    int64_t gt_off = 0;
    for (size_t k = 0; k < tr->det_convs.size(); ++k) {
        const TConv& c = tr->convs[tr->det_convs[k]];
        const Layer& l = h->layers[c.layer];
        if (l.det_kind == BYOLO_DET_EPISTEMIC) return fail(h, BYOLO_ERR_ARG, "byolo_trainer_step: epistemic detection layers have no loss (inference_mode=False)");
        const TTensor& t = tr->tens[c.out];
        rc = byolo_loss(h, l.det_kind, tr->aleatoric_loss, h->cfg.cls_cnt, F(t.act), c.Cout, B, l.H, l.W, d_gt_loc + 4 * gt_off, d_gt_obj + gt_off,
                        d_gt_cls + gt_off, d_gt_ign + gt_off, N_all, reinterpret_cast<double*>(ws + tr->ws_loss) + 3 * k, F(t.grad), c.Cout,
                        ws + tr->ws_lossws, byolo_loss_workspace_bytes(), st);
        if (rc) return rc;
        gt_off += (int64_t)l.H * l.W * 3;
    }
    hipLaunchKernelGGL(sumsq_partial, dim3(RED_BLOCKS), dim3(256), 0, st, tr->d_w, tr->n_l2, reinterpret_cast<double*>(ws + tr->ws_sq));
    hipLaunchKernelGGL(losses_kernel, dim3(1), dim3(64), 0, st, reinterpret_cast<const double*>(ws + tr->ws_loss), (int)tr->det_convs.size(),
                       reinterpret_cast<const double*>(ws + tr->ws_sq), RED_BLOCKS, tr->reg_const, (double)L2_SCALE, d_losses);
    HIPCHK(h, hipGetLastError());
    // ---- backward, layers in reverse order: the first contribution to a tensor's gradient writes it, later ones add ---------
    for (auto& t : tr->tens) t.grad_set = false;
    for (int ci : tr->det_convs) tr->tens[tr->convs[ci].out].grad_set = true;
    for (int i = (int)tr->convs.size() - 1; i >= 0; --i) {
        TConv& c = tr->convs[i];
        const Layer& l = h->layers[c.layer];
        const int64_t M = (int64_t)B * l.H * l.W;
        TTensor& o = tr->tens[c.out];
        if (!o.grad_set) return fail(h, BYOLO_ERR_ARG, "byolo_trainer_step: the output of head layer '%s' reaches no loss", l.scope.c_str());
        float* dz = F(o.grad);
        float* gk = tr->d_g + tr->vars[c.v_kernel].off;
        if (c.det) {
            hipLaunchKernelGGL(colsum_partial, dim3(RED_BLOCKS), dim3(256), 0, st, dz, M, c.Cout, tmp);
            hipLaunchKernelGGL(bn_bwd_final, dim3((c.Cout + 255) / 256), dim3(256), 0, st, tmp, RED_BLOCKS, M, c.Cout, nullptr,
                               tr->d_g + tr->vars[c.v_bias].off, nullptr);
        } else {
            const float* gam = tr->d_w + tr->vars[c.v_gamma].off; const float* bet = tr->d_w + tr->vars[c.v_beta].off;
            float* k12 = F(tr->ws_k12);
            hipLaunchKernelGGL(bn_bwd_partial, dim3(RED_BLOCKS), dim3(256), 0, st, dz, F(c.z), M, c.Cout, bmean + c.mov_off, bvar + c.mov_off, gam, bet, tmp);
            hipLaunchKernelGGL(bn_bwd_final, dim3((c.Cout + 255) / 256), dim3(256), 0, st, tmp, RED_BLOCKS, M, c.Cout,
                               tr->d_g + tr->vars[c.v_gamma].off, tr->d_g + tr->vars[c.v_beta].off, k12);
            hipLaunchKernelGGL(bn_bwd_apply, dim3(grid1d(M * c.Cout)), dim3(256), 0, st, dz, F(c.z), M * c.Cout, c.Cout, bmean + c.mov_off,
                               bvar + c.mov_off, gam, bet, k12, drop_of(c));
        }
        HIPCHK(h, hipGetLastError());
        // wgrad: dW[(tap, ci)][co] = sum over pixels of im2col(x)[pixel][(tap, ci)] * dz[pixel][co]
        const int64_t Kc = (int64_t)c.ks * c.ks * c.Cin;
        GemmArgs wa; memset(&wa, 0, sizeof wa);
        wa.mode = 1; wa.x = input_ptr(c); wa.S = B; wa.H = l.H; wa.W = l.W; wa.Cin = c.Cin; wa.ks = c.ks; wa.pad = c.ks == 3 ? 1 : 0;
        wa.b = dz; wa.N = c.Cout; wa.c = F(tr->ws_partial); wa.ldc = c.Cout; wa.Mo = (int)Kc; wa.Kred = (int)M;
        wa.kslice = c.kslice; wa.pstride = (size_t)Kc * c.Cout;
        HIPCHK(h, launch_gemm(wa, c.slices, GEMM_WGRAD, st));
        hipLaunchKernelGGL(combine_slices_kernel, dim3(grid1d(Kc * c.Cout)), dim3(256), 0, st, F(tr->ws_partial), c.slices, wa.pstride, Kc * c.Cout, gk);
        if (!c.in_grad) continue;
        // dgrad: dx = conv(dz, rotated W) -- straight into the input tensor's gradient, or into dx of the concat, then split
        hipLaunchKernelGGL(rotate_kernel, dim3(grid1d(Kc * c.Cout)), dim3(256), 0, st, tr->d_w + tr->vars[c.v_kernel].off, tr->d_wt, c.ks, c.Cin, c.Cout);
        if (!c.xbuf) {
            TTensor& it = tr->tens[c.in[0].tensor];
            GemmArgs da = conv_args(dz, B, l.H, l.W, c.Cout, c.ks, tr->d_wt, c.Cin, F(it.grad));
            da.accumulate = it.grad_set ? 1 : 0;
            HIPCHK(h, launch_gemm(da, 1, GEMM_DGRAD, st));
            it.grad_set = true;
        } else {
            GemmArgs da = conv_args(dz, B, l.H, l.W, c.Cout, c.ks, tr->d_wt, c.Cin, F(c.dx));
            HIPCHK(h, launch_gemm(da, 1, GEMM_DGRAD, st));
            int c_off = 0;
            for (auto& p : c.in) {
                TTensor& it = tr->tens[p.tensor];
                if (!it.frozen) {
                    const int64_t n = (int64_t)B * (l.H >> p.sh) * (l.W >> p.sh) * p.C;
                    hipLaunchKernelGGL(scatter_kernel, dim3(grid1d(n)), dim3(256), 0, st, F(c.dx), B, l.H, l.W, c.Cin, c_off, p.C, p.sh,
                                       F(it.grad), it.grad_set ? 1 : 0);
                    it.grad_set = true;
                }
                c_off += p.C;
            }
            HIPCHK(h, hipGetLastError());
        }
    }
    // ---- update: L2 gradient + Adam over the flat buffer, then the moving statistics ------------------------------------------
    const int update = grads_only ? 0 : 1;
    const double t1 = (double)(tr->step + 1);
    const float lr_t = (float)((double)lr * std::sqrt(1.0 - std::pow(ADAM_B2, t1)) / (1.0 - std::pow(ADAM_B1, t1)));
    hipLaunchKernelGGL(adam_kernel, dim3(grid1d(tr->n_flat)), dim3(256), 0, st, tr->d_w, tr->d_g, tr->d_m, tr->d_v, tr->n_flat, tr->n_l2,
                       L2_SCALE, update, lr_t, (float)(1.0 - ADAM_B1), (float)(1.0 - ADAM_B2), ADAM_EPS);
    if (update && tr->n_mov) {
        hipLaunchKernelGGL(moving_kernel, dim3(grid1d(tr->n_mov)), dim3(256), 0, st, tr->d_mov, bmean, tr->n_mov, BN_DECAY);
        hipLaunchKernelGGL(moving_kernel, dim3(grid1d(tr->n_mov)), dim3(256), 0, st, tr->d_mov + tr->n_mov, bvaru, tr->n_mov, BN_DECAY);
    }
    HIPCHK(h, hipGetLastError());
    if (update) ++tr->step;
    return BYOLO_OK;
}

extern "C" int32_t byolo_trainer_step(byolo_trainer_t* tr, const float* d_img, int32_t B, uint64_t seed, const uint32_t* d_mask_bits,
                                      const float* d_gt_loc, const float* d_gt_obj, const int32_t* d_gt_cls, const float* d_gt_ign, float lr,
                                      int32_t grads_only, double* d_losses, void* d_workspace, size_t workspace_bytes, void* stream) {
    if (!tr) return fail(nullptr, BYOLO_ERR_ARG, "byolo_trainer_step: null trainer");
    return guarded(tr->h, "byolo_trainer_step", [&] {
        return trainer_step_impl(tr, d_img, B, seed, d_mask_bits, d_gt_loc, d_gt_obj, d_gt_cls, d_gt_ign, lr, grads_only, d_losses,
                                 d_workspace, workspace_bytes, stream);
    });
}

extern "C" int32_t byolo_trainer_num_vars(const byolo_trainer_t* tr) { return tr ? (int32_t)tr->vars.size() : BYOLO_ERR_ARG; }

extern "C" int32_t byolo_trainer_var_info(const byolo_trainer_t* tr, int32_t i, const char** name, int32_t* ndim, int64_t shape[4]) {
    if (!tr || i < 0 || i >= (int)tr->vars.size()) return fail(tr ? tr->h : nullptr, BYOLO_ERR_ARG, "byolo_trainer_var_info: bad index");
    const TVar& v = tr->vars[i];
    if (name) *name = v.name.c_str();
    if (ndim) *ndim = (int32_t)v.shape.size();
    if (shape) for (size_t k = 0; k < 4; ++k) shape[k] = k < v.shape.size() ? v.shape[k] : 1;
    return BYOLO_OK;
}

// name -> (device pointer, count): trainable tensors in slots 0 value / 1 gradient / 2 Adam / 3 Adam_1, moving statistics in slot 0
static int32_t locate(byolo_trainer_t* tr, const char* name, int32_t slot, float** p, int64_t* n) {
    if (!name || slot < 0 || slot > 3) return tfail(tr, BYOLO_ERR_ARG, "byolo_trainer_get / _set: bad name or slot");
    if (int32_t rc = trainer_device(tr)) return rc;
    auto it = tr->vindex.find(name);
    if (it != tr->vindex.end()) {
        const TVar& v = tr->vars[it->second];
        float* base[4] = {tr->d_w, tr->d_g, tr->d_m, tr->d_v};
        *p = base[slot] + v.off; *n = v.n;
        return BYOLO_OK;
    }
    const std::string s(name);
    for (auto& c : tr->convs) {
        if (c.det) continue;
        const Layer& l = tr->h->layers[c.layer];
        for (int k = 0; k < 2; ++k) {
            if (s == tr->h->params[k ? l.p_var : l.p_mean].name) {
                if (slot) return fail(tr->h, BYOLO_ERR_ARG, "byolo_trainer_get / _set: '%s' is a moving statistic (slot 0 only)", name);
                *p = tr->d_mov + (k ? tr->n_mov : 0) + c.mov_off; *n = c.Cout;
                return BYOLO_OK;
            }
        }
    }
    return fail(tr->h, BYOLO_ERR_ARG, "byolo_trainer_get / _set: '%s' is not a variable of the trained heads", name);
}

extern "C" int32_t byolo_trainer_get(byolo_trainer_t* tr, const char* name, int32_t slot, float* h_data, int64_t count) {
    if (!tr || !h_data) return fail(tr ? tr->h : nullptr, BYOLO_ERR_ARG, "byolo_trainer_get: null argument");
    float* p; int64_t n;
    int32_t rc = locate(tr, name, slot, &p, &n); if (rc) return rc;
    if (count != n) return fail(tr->h, BYOLO_ERR_ARG, "byolo_trainer_get: '%s' has %lld values, asked for %lld", name, (long long)n, (long long)count);
    HIPCHK(tr->h, hipSetDevice(tr->device));
    HIPCHK(tr->h, hipDeviceSynchronize());
    HIPCHK(tr->h, hipMemcpy(h_data, p, sizeof(float) * n, hipMemcpyDeviceToHost));
    return BYOLO_OK;
}

extern "C" int32_t byolo_trainer_set(byolo_trainer_t* tr, const char* name, int32_t slot, const float* h_data, int64_t count) {
    if (!tr || !h_data) return fail(tr ? tr->h : nullptr, BYOLO_ERR_ARG, "byolo_trainer_set: null argument");
    float* p; int64_t n;
    int32_t rc = locate(tr, name, slot, &p, &n); if (rc) return rc;
    if (count != n) return fail(tr->h, BYOLO_ERR_ARG, "byolo_trainer_set: '%s' has %lld values, got %lld", name, (long long)n, (long long)count);
    HIPCHK(tr->h, hipSetDevice(tr->device));
    HIPCHK(tr->h, hipDeviceSynchronize());
    HIPCHK(tr->h, hipMemcpy(p, h_data, sizeof(float) * n, hipMemcpyHostToDevice));
    return BYOLO_OK;
}

extern "C" int32_t byolo_trainer_get_step(const byolo_trainer_t* tr, int64_t* step) {
    if (!tr || !step) return fail(tr ? tr->h : nullptr, BYOLO_ERR_ARG, "byolo_trainer_get_step: null argument");
    *step = tr->step;
    return BYOLO_OK;
}

extern "C" int32_t byolo_trainer_set_step(byolo_trainer_t* tr, int64_t step) {
    if (!tr || step < 0) return fail(tr ? tr->h : nullptr, BYOLO_ERR_ARG, "byolo_trainer_set_step: bad argument");
    tr->step = step;
    return BYOLO_OK;
}

extern "C" int32_t byolo_trainer_export(byolo_trainer_t* tr, byolo_t* dst) {
    if (!tr || !dst) return fail(tr ? tr->h : nullptr, BYOLO_ERR_ARG, "byolo_trainer_export: null argument");
    return guarded(tr->h, "byolo_trainer_export", [&] {
        std::vector<float> buf;
        std::vector<std::string> names;
        for (auto& v : tr->vars) names.push_back(v.name);
        for (auto& c : tr->convs) if (!c.det) {
            const Layer& l = tr->h->layers[c.layer];
            names.push_back(tr->h->params[l.p_mean].name); names.push_back(tr->h->params[l.p_var].name);
        }
        for (auto& nm : names) {
            float* p; int64_t n;
            int32_t rc = locate(tr, nm.c_str(), 0, &p, &n); if (rc) return rc;
            buf.resize((size_t)n);
            HIPCHK(tr->h, hipSetDevice(tr->device));
            HIPCHK(tr->h, hipDeviceSynchronize());
            HIPCHK(tr->h, hipMemcpy(buf.data(), p, sizeof(float) * n, hipMemcpyDeviceToHost));
            rc = byolo_set_param(dst, nm.c_str(), buf.data(), n);
            if (rc) return fail(tr->h, rc, "byolo_trainer_export: %s", dst->err.c_str());
        }
        dst->finalized = false;                              // the caller finalizes dst to run inference with the new weights
        return (int32_t)BYOLO_OK;
    });
}

extern "C" int32_t byolo_trainer_taps(const byolo_trainer_t* tr, int32_t* layers, int32_t cap) {
    if (!tr) return fail(nullptr, BYOLO_ERR_ARG, "byolo_trainer_taps: null trainer");
    for (int k = 0; k < (int)tr->taps.size() && k < cap && layers; ++k) layers[k] = tr->tens[tr->taps[k]].layer;
    return (int32_t)tr->taps.size();
}

extern "C" int32_t byolo_trainer_layer_output(byolo_trainer_t* tr, int32_t layer, float* d_dst, int64_t count, int64_t shape[4], void* stream) {
    if (!tr) return fail(nullptr, BYOLO_ERR_ARG, "byolo_trainer_layer_output: null trainer");
    for (auto& t : tr->tens) {
        if (t.layer != layer) continue;
        const int B = tr->ws_B;
        if (shape) { shape[0] = B; shape[1] = t.H; shape[2] = t.W; shape[3] = t.C; }
        if (!d_dst) return BYOLO_OK;
        if (!tr->last_ws || B < 1) return tfail(tr, BYOLO_ERR_STATE, "byolo_trainer_layer_output: no step has run");
        const int64_t n = (int64_t)B * t.H * t.W * t.C;
        if (count != n) return fail(tr->h, BYOLO_ERR_ARG, "byolo_trainer_layer_output: layer %d has %lld values, asked for %lld", layer, (long long)n, (long long)count);
        HIPCHK(tr->h, hipMemcpyAsync(d_dst, reinterpret_cast<char*>(tr->last_ws) + t.act, (size_t)n * 4, hipMemcpyDeviceToDevice,
                                     reinterpret_cast<hipStream_t>(stream)));
        return BYOLO_OK;
    }
    return fail(tr->h, BYOLO_ERR_ARG, "byolo_trainer_layer_output: layer %d is neither a tap nor a head convolution", layer);
}
