// augment.hip -- the training feed's crop and augmentation (include/byolo.h byolo_augment_batch): lib_yolo/data_augmentation.py's
// ImageCropper (:139-228) and DataAugmenter.augment (:20-133) over the decoded uint8 frames of a batch, in one launch.
//
// Per output element (image b, row i, column j, channel c), in this order -- every float32 operation is the one written here, in
// this order (the file is compiled with contraction off and correctly rounded division, csrc/build.py FILE_FLAGS), so that
// tests/_augment_ref.py restates it bit for bit:
//   1. C(y, x)  = float(u8[y0 + y][x0 + x][c]) * (1.0f / 255.0f)                               (decode_img; byolo_normalize_u8)
//   2. R(i, x)  = C(i, x), or with `rescale` TF1's legacy ResizeBilinear CPU kernel from ch x cw to out_h x out_w:
//                 s = float(ch) / float(out_h); in = float(i) * s; lo = max(floor(in), 0); hi = min(ceil(in), ch - 1);
//                 l = in - floor(in) (the same along x); top = tl + (tr - tl) * lx; bottom = bl + (br - bl) * lx;
//                 R = top + (bottom - top) * ly
//   3. F(i, j)  = R(i, out_w - 1 - j) with `flip`, else R(i, j)
//   4. blur k   acc = 0; for dy < k, for dx < k: acc = acc + F(i + dy - p, j + dx - p) * w, p = (k - 1) / 2, w = 1.0f / float(k * k),
//               F = 0 outside the image (conv2d SAME, zero padding: k = 2 pads nothing before and one pixel after)
//   5. colour   per pixel: TF's AdjustSaturation (rgb -> hsv, s * factor clamped to [0, 1], hsv -> rgb), brightness (+ delta) or
//               AdjustHue (hue in [0, 6), h += 6 * delta wrapped, the pixel's min and max kept); no clipping afterwards
//   6. noise    coloured salt and pepper (per element: 1 if U(e, SALT) < amount; then 0 if U(e, PEPPER) < amount), salt and
//               pepper (per pixel: + (U(p, SALT) < amount) - (U(p, PEPPER) < amount) on all three channels, then EVERY element
//               clipped to [0, 1]) or Gaussian (+ stddev * N(e)), e = (i * out_w + j) * 3 + c, p = i * out_w + j.
//
// The noise stream.  The reference draws its masks from TF's unseeded generator; the build defines them as a pure function of the
// image's 64-bit noise key (byolo/augment.py draws it with the plan) and the element:
//   hash(key, n, purpose) = x after   x = lowbias32(n + lo32(key));  x ^= hi32(key) + purpose * 0x9E3779B9;  x = lowbias32(x)
//   U(n, purpose)         = float(hash >> 8) * 2^-24                                               (in [0, 1 - 2^-24], exact)
//   N(n)                  = sqrtf(-2 * logf(1 - U(n, GAUSS_1))) * cosf(6.2831855f * U(n, GAUSS_2))    (Box-Muller, accurate libm)
// with lowbias32 = byolo_mix32 (byolo_rng.h) and purposes SALT 1, PEPPER 2, GAUSS_1 3, GAUSS_2 4.  The Gaussian term is the only
// one whose last bits depend on the libm (logf / cosf); everything else is exact.
//
// Shape: a workgroup (256 threads) owns a 16 x 64 pixel tile of one image, so every per-image branch is uniform.  Phase 1 writes F
// of the tile (plus a one-pixel halo when the image blurs) to LDS; phase 2 blurs from LDS and applies the colour and noise ops per
// pixel into a second LDS tile; phase 3 writes the tile's rows with 16-byte stores over the aligned part of each row (scalar stores
// at the row's two ends only).
#include "byolo_internal.h"
#include "byolo_rng.h"

#pragma clang fp contract(off)

namespace {

constexpr int TH = 16, TW = 64, NT = 256;
constexpr int HALO_W = TW + 2, HALO_H = TH + 2;
constexpr int CHUNK = 32;                           // images per launch: the plans travel as a kernel argument (32 x 56 bytes)
constexpr uint32_t P_SALT = 1, P_PEPPER = 2, P_GAUSS_1 = 3, P_GAUSS_2 = 4;

struct PlanChunk { byolo_aug_plan p[CHUNK]; };

__device__ __forceinline__ uint32_t aug_hash(uint64_t key, uint32_t n, uint32_t purpose) {
    uint32_t x = byolo_mix32(n + (uint32_t)key);
    x ^= (uint32_t)(key >> 32) + purpose * 0x9E3779B9u;
    return byolo_mix32(x);
}
__device__ __forceinline__ float aug_uniform(uint64_t key, uint32_t n, uint32_t purpose) {
    return (float)(aug_hash(key, n, purpose) >> 8) * 5.9604644775390625e-08f;          // 2^-24
}

// TF adjust_saturation_op.cc (CPU): rgb_to_hsv / hsv_to_rgb, including its double-precision hue offsets
__device__ void adjust_saturation(float& r, float& g, float& b, float factor) {
    const float vv = fmaxf(r, fmaxf(g, b));
    const float range = vv - fminf(r, fminf(g, b));
    float s = vv > 0.f ? range / vv : 0.f;
    const float norm = 1.0f / (6.0f * range);
    float hh;
    if (r == vv) hh = norm * (g - b);
    else if (g == vv) hh = (float)((double)(norm * (b - r)) + 2.0 / 6.0);
    else hh = (float)((double)(norm * (r - g)) + 4.0 / 6.0);
    if (range <= 0.f) hh = 0.f;
    if (hh < 0.f) hh = hh + 1.0f;
    s = fminf(1.0f, fmaxf(0.0f, s * factor));
    const float c = s * vv, m = vv - c, dh = hh * 6.0f;
    const int cat = (int)dh;
    float fm = dh;
    while (fm <= 0.f) fm += 2.0f;
    while (fm >= 2.0f) fm -= 2.0f;
    const float x = c * (1.0f - fabsf(fm - 1.0f));
    float rr, gg, bb;
    switch (cat) {
        case 0: rr = c; gg = x; bb = 0.f; break;
        case 1: rr = x; gg = c; bb = 0.f; break;
        case 2: rr = 0.f; gg = c; bb = x; break;
        case 3: rr = 0.f; gg = x; bb = c; break;
        case 4: rr = x; gg = 0.f; bb = c; break;
        case 5: rr = c; gg = 0.f; bb = x; break;
        default: rr = 0.f; gg = 0.f; bb = 0.f;
    }
    r = rr + m; g = gg + m; b = bb + m;
}

// TF adjust_hue_op.cc (CPU): rgb_to_hv_range / hv_range_to_rgb
__device__ void adjust_hue(float& r, float& g, float& b, float delta) {
    float vmax, vmid, vmin;
    int cat;
    if (r < g) {
        if (b < r) { vmax = g; vmid = r; vmin = b; cat = 1; }
        else if (b > g) { vmax = b; vmid = g; vmin = r; cat = 3; }
        else { vmax = g; vmid = b; vmin = r; cat = 2; }
    } else {
        if (b < g) { vmax = r; vmid = g; vmin = b; cat = 0; }
        else if (b > r) { vmax = b; vmid = r; vmin = g; cat = 4; }
        else { vmax = r; vmid = b; vmin = g; cat = 5; }
    }
    float h;
    if (vmax == vmin) {
        h = 0.f;
    } else {
        const float ratio = (vmid - vmin) / (vmax - vmin);
        h = (float)cat + ((cat & 1) == 0 ? ratio : (1.0f - ratio));
    }
    h = h + delta * 6.0f;
    while (h < 0.f) h = h + 6.0f;
    while (h >= 6.0f) h = h - 6.0f;
    const int hc = (int)h;
    float ratio = h - (float)hc;
    if (hc & 1) ratio = 1.0f - ratio;
    const float mid = vmin + ratio * (vmax - vmin);
    switch (hc) {
        case 0: r = vmax; g = mid; b = vmin; break;
        case 1: r = mid; g = vmax; b = vmin; break;
        case 2: r = vmin; g = vmax; b = mid; break;
        case 3: r = vmin; g = mid; b = vmax; break;
        case 4: r = mid; g = vmin; b = vmax; break;
        default: r = vmax; g = vmin; b = mid;
    }
}

__global__ __launch_bounds__(NT) void augment_kernel(const uint8_t* __restrict__ src, int64_t img_stride, int32_t src_w,
                                                     PlanChunk plans, int32_t out_h, int32_t out_w, float* __restrict__ out) {
    __shared__ float sF[HALO_H * HALO_W * 3];
    __shared__ float sO[TH * TW * 3];
    const byolo_aug_plan& P = plans.p[blockIdx.z];
    const int tid = threadIdx.x;
    const int i0 = blockIdx.y * TH, j0 = blockIdx.x * TW;
    const uint8_t* img = src + (int64_t)blockIdx.z * img_stride;
    const int64_t row_bytes = (int64_t)src_w * 3;
    const int ybase = P.y0 - P.row0, x0 = P.x0, ch = P.ch, cw = P.cw;
    const float K = 1.0f / 255.0f;
    const int halo = P.blur_k ? 1 : 0;
    const float hs = (float)ch / (float)out_h, ws = (float)cw / (float)out_w;

    // phase 1: F over the tile (+ halo) -> sF[(li + 1) * HALO_W + (lj + 1)][c]
    const int hh = TH + 2 * halo, hw = TW + 2 * halo;
    for (int q = tid; q < hh * hw; q += NT) {
        const int li = q / hw - halo, lj = q % hw - halo;
        const int i = i0 + li, j = j0 + lj;
        float v[3] = {0.f, 0.f, 0.f};
        if (i >= 0 && i < out_h && j >= 0 && j < out_w) {
            const int jj = P.flip ? out_w - 1 - j : j;
            if (!P.rescale) {
                const uint8_t* s = img + (int64_t)(ybase + i) * row_bytes + (int64_t)(x0 + jj) * 3;
                for (int c = 0; c < 3; ++c) v[c] = (float)s[c] * K;
            } else {
                const float iny = (float)i * hs, fy = floorf(iny);
                const float inx = (float)jj * ws, fx = floorf(inx);
                const int ylo = min(max((int)fy, 0), ch - 1), yhi = min((int)ceilf(iny), ch - 1);
                const int xlo = min(max((int)fx, 0), cw - 1), xhi = min((int)ceilf(inx), cw - 1);
                const float ly = iny - fy, lx = inx - fx;
                const uint8_t* rt = img + (int64_t)(ybase + ylo) * row_bytes;
                const uint8_t* rb = img + (int64_t)(ybase + yhi) * row_bytes;
                const int64_t cl = (int64_t)(x0 + xlo) * 3, cr = (int64_t)(x0 + xhi) * 3;
                for (int c = 0; c < 3; ++c) {
                    const float tl = (float)rt[cl + c] * K, tr = (float)rt[cr + c] * K;
                    const float bl = (float)rb[cl + c] * K, br = (float)rb[cr + c] * K;
                    const float top = tl + (tr - tl) * lx;
                    const float bottom = bl + (br - bl) * lx;
                    v[c] = top + (bottom - top) * ly;
                }
            }
        }
        float* d = sF + ((li + 1) * HALO_W + (lj + 1)) * 3;
        d[0] = v[0]; d[1] = v[1]; d[2] = v[2];
    }
    __syncthreads();

    // phase 2: blur, colour, noise per pixel -> sO
    const int k = P.blur_k, pad = (k - 1) / 2;
    const float w = k ? 1.0f / (float)(k * k) : 0.f;
    for (int q = tid; q < TH * TW; q += NT) {
        const int li = q / TW, lj = q % TW;
        const int i = i0 + li, j = j0 + lj;
        if (i >= out_h || j >= out_w) continue;
        float v[3];
        if (k) {
            for (int c = 0; c < 3; ++c) {
                float acc = 0.f;
                for (int dy = 0; dy < k; ++dy)
                    for (int dx = 0; dx < k; ++dx)
                        acc = acc + sF[((li + 1 + dy - pad) * HALO_W + (lj + 1 + dx - pad)) * 3 + c] * w;
                v[c] = acc;
            }
        } else {
            const float* s = sF + ((li + 1) * HALO_W + (lj + 1)) * 3;
            v[0] = s[0]; v[1] = s[1]; v[2] = s[2];
        }
        if (P.color_op == BYOLO_AUG_SATURATION) adjust_saturation(v[0], v[1], v[2], P.color_param);
        else if (P.color_op == BYOLO_AUG_BRIGHTNESS) { v[0] = v[0] + P.color_param; v[1] = v[1] + P.color_param; v[2] = v[2] + P.color_param; }
        else if (P.color_op == BYOLO_AUG_HUE) adjust_hue(v[0], v[1], v[2], P.color_param);
        const uint32_t pix = (uint32_t)i * (uint32_t)out_w + (uint32_t)j;
        if (P.noise_op == BYOLO_AUG_COLORED_SALT_N_PEPPER) {
            for (int c = 0; c < 3; ++c) {
                const uint32_t e = pix * 3u + (uint32_t)c;
                if (aug_uniform(P.noise_key, e, P_SALT) < P.noise_param) v[c] = 1.0f;
                if (aug_uniform(P.noise_key, e, P_PEPPER) < P.noise_param) v[c] = 0.0f;
            }
        } else if (P.noise_op == BYOLO_AUG_SALT_N_PEPPER) {
            const float salt = aug_uniform(P.noise_key, pix, P_SALT) < P.noise_param ? 1.0f : 0.0f;
            const float pepper = aug_uniform(P.noise_key, pix, P_PEPPER) < P.noise_param ? -1.0f : 0.0f;
            const float snp = salt + pepper;
            for (int c = 0; c < 3; ++c) v[c] = fmaxf(fminf(v[c] + snp, 1.0f), 0.0f);
        } else if (P.noise_op == BYOLO_AUG_GAUSSIAN) {
            for (int c = 0; c < 3; ++c) {
                const uint32_t e = pix * 3u + (uint32_t)c;
                const float u1 = 1.0f - aug_uniform(P.noise_key, e, P_GAUSS_1);
                const float u2 = aug_uniform(P.noise_key, e, P_GAUSS_2);
                const float z = sqrtf(-2.0f * logf(u1)) * cosf(6.2831855f * u2);
                v[c] = v[c] + z * P.noise_param;
            }
        }
        float* d = sO + (li * TW + lj) * 3;
        d[0] = v[0]; d[1] = v[1]; d[2] = v[2];
    }
    __syncthreads();

    // phase 3: rows of the tile -> out, 16-byte stores on the 16-byte slots a row covers completely
    const int ncols = min(TW, out_w - j0), n = ncols * 3;
    float* oimg = out + (int64_t)blockIdx.z * out_h * out_w * 3;
    constexpr int SLOTS = TW * 3 / 4 + 1;
    for (int q = tid; q < TH * SLOTS; q += NT) {
        const int li = q / SLOTS, sl = q % SLOTS;
        const int i = i0 + li;
        if (i >= out_h) continue;
        float* row = oimg + ((int64_t)i * out_w + j0) * 3;
        const int lead = (int)((reinterpret_cast<uintptr_t>(row) & 15) >> 2);        // elements before the first 16-byte boundary
        const int e0 = sl * 4 - lead;                                                 // first element of this slot (may be < 0)
        if (e0 >= n) continue;
        const float* s = sO + li * TW * 3;
        if (e0 >= 0 && e0 + 4 <= n) {
            float4 v = make_float4(s[e0], s[e0 + 1], s[e0 + 2], s[e0 + 3]);
            *reinterpret_cast<float4*>(row + e0) = v;
        } else {
            for (int u = 0; u < 4; ++u) {
                const int e = e0 + u;
                if (e >= 0 && e < n) row[e] = s[e];
            }
        }
    }
}

}  // namespace

extern "C" int32_t byolo_augment_batch(byolo_t* h, const uint8_t* d_u8, int32_t B, int32_t src_h, int32_t src_w, int64_t img_stride,
                                       const byolo_aug_plan* h_plans, int32_t out_h, int32_t out_w, float* d_out, void* stream) {
    if (B < 0 || src_h < 1 || src_w < 1 || out_h < 1 || out_w < 1 || (B > 0 && (!d_u8 || !h_plans || !d_out)))
        return fail(h, BYOLO_ERR_ARG, "byolo_augment_batch: bad argument");
    if (img_stride < (int64_t)src_h * src_w * 3 || (int64_t)out_h * out_w * 3 >= ((int64_t)1 << 31) ||
        (int64_t)src_h * src_w * 3 >= ((int64_t)1 << 40))
        return fail(h, BYOLO_ERR_ARG, "byolo_augment_batch: img_stride below src_h * src_w * 3 bytes, or sizes out of range");
    if (reinterpret_cast<uintptr_t>(d_out) & 3) return fail(h, BYOLO_ERR_ARG, "byolo_augment_batch: d_out must be 4-byte aligned");
    for (int32_t b = 0; b < B; ++b) {
        const byolo_aug_plan& p = h_plans[b];
        const bool window = p.ch >= 1 && p.cw >= 1 && p.x0 >= 0 && p.row0 >= 0 && p.y0 >= p.row0 &&
                            (int64_t)p.y0 - p.row0 + p.ch <= src_h && (int64_t)p.x0 + p.cw <= src_w;
        if (!window)
            return fail(h, BYOLO_ERR_ARG, "byolo_augment_batch: image %d: window y0 %d x0 %d %d x %d (row0 %d) outside the %d x %d rows shipped",
                        b, p.y0, p.x0, p.ch, p.cw, p.row0, src_h, src_w);
        if ((p.rescale != 0 && p.rescale != 1) || (p.flip != 0 && p.flip != 1))
            return fail(h, BYOLO_ERR_ARG, "byolo_augment_batch: image %d: rescale / flip must be 0 or 1", b);
        if (!p.rescale && (p.ch != out_h || p.cw != out_w))
            return fail(h, BYOLO_ERR_ARG, "byolo_augment_batch: image %d: a window of %d x %d without rescale cannot fill %d x %d",
                        b, p.ch, p.cw, out_h, out_w);
        if (p.blur_k != 0 && p.blur_k != 2 && p.blur_k != 3)
            return fail(h, BYOLO_ERR_ARG, "byolo_augment_batch: image %d: blur_k %d is not 0, 2 or 3", b, p.blur_k);
        if (p.color_op < BYOLO_AUG_COLOR_NONE || p.color_op > BYOLO_AUG_HUE || p.noise_op < BYOLO_AUG_NOISE_NONE ||
            p.noise_op > BYOLO_AUG_GAUSSIAN)
            return fail(h, BYOLO_ERR_ARG, "byolo_augment_batch: image %d: unknown colour op %d or noise op %d", b, p.color_op, p.noise_op);
        // the hue op wraps h into [0, 6) by whole turns, as TF's kernel does: a delta outside tf.image.adjust_hue's [-1, 1] (or
        // a non-finite one) would turn those loops into millions of iterations per pixel, or into loops that never end
        if (!std::isfinite(p.color_param) || !std::isfinite(p.noise_param) ||
            (p.color_op == BYOLO_AUG_HUE && !(p.color_param >= -1.0f && p.color_param <= 1.0f)))
            return fail(h, BYOLO_ERR_ARG, "byolo_augment_batch: image %d: colour parameter %g or noise parameter %g out of range "
                        "(finite; a hue delta in [-1, 1])", b, (double)p.color_param, (double)p.noise_param);
    }
    if (B == 0) return BYOLO_OK;
    if (h) HIPCHK(h, hipSetDevice(h->device));
    const hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const dim3 block(NT);
    for (int32_t b0 = 0; b0 < B; b0 += CHUNK) {
        const int n = std::min(CHUNK, B - b0);
        PlanChunk pc;
        memset(&pc, 0, sizeof pc);
        memcpy(pc.p, h_plans + b0, sizeof(byolo_aug_plan) * n);
        const dim3 grid((out_w + TW - 1) / TW, (out_h + TH - 1) / TH, n);
        hipLaunchKernelGGL(augment_kernel, grid, block, 0, st, d_u8 + (int64_t)b0 * img_stride, img_stride, src_w, pc, out_h, out_w,
                           d_out + (int64_t)b0 * out_h * out_w * 3);
        HIPCHK(h, hipGetLastError());
    }
    return BYOLO_OK;
}
