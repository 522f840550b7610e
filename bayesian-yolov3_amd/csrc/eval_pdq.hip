// eval_pdq.hip -- probabilistic detection quality (Hall et al., "Probabilistic Object Detection: Definition and Evaluation",
// WACV 2020) behind the evaluator's matching (include/byolo.h byolo_eval_set_pdq; INTEGRATION.md "Evaluation" has the definition,
// tests/_pdq_ref.py restates it in numpy).  Three launches per byolo_eval_add on the caller's stream, no host wait; everything
// between them lives in a caller-owned workspace, one slice per image of the batch:
//
//   pdq_list_kernel    one workgroup per image.  The image's detections -- rows whose score (class and score by the rule of the main
//                      table) is finite and >= min_score -- as sorted keys in LDS (descending score, then ascending row: the main
//                      matching's order), and per detection the corner means in pixels and the two standard deviations: the
//                      variances of the raw location values go to box units as the variance voting takes them there, all float64.
//                      The counted ground-truth boxes (a class label, a non-empty pixel rectangle) are compacted in ascending index
//                      with their rectangles.
//   pdq_pair_kernel    one workgroup per (image, detection).  px[u] and py[v] of the whole frame are staged in LDS, (img_w + img_h)
//                      doubles; the support [u0, u1) x [v0, v1) is where they reach p_min (p = px py <= min(px, py), so the segment
//                      {p >= p_min} lies inside it).  Then the counted boxes in turn: one that misses the support costs five zeros,
//                      the others two passes with the lanes over pixels -- the box inside the support for L_FG (the box's pixels
//                      outside it are log(eps) each and are counted, not visited), the support without the box for L_BG, which is
//                      evaluated directly over segment \ box.  Every sum: a lane adds its pixels in ascending order, the 64 lanes
//                      fold by a butterfly, the four waves in ascending order -- the same bits in every run.
//   pdq_assign_kernel  one workgroup per image: the shortest-augmenting-path Hungarian method with row and column potentials on
//                      cost = -pPDQ, the smaller side as rows.  Potentials, minv, way, used and the matching are in LDS; thread t
//                      owns the columns t + 1, t + 257, t + 513, t + 769, one workgroup arg-min per step with ties to the lowest
//                      column.  Only float64 add, subtract and compare: on the same matrix it is tests/_pdq_ref.py bit for bit.
//                      The image's record goes to index (image sequence number) of the image table, its true positives to the
//                      pair table behind an atomic cursor; a record that does not fit raises a flag and is not written.
//
// No run-time-indexed per-lane arrays: no private segment (tests/test_no_scratch.py).
#include "eval_pdq.h"

#include <cfloat>
#include <cstring>

#include "nms_box.h"

namespace byk {

static constexpr int PDQ_MAX_DET = BYOLO_PDQ_MAX_DET;
static constexpr int PDQ_NT = 256;                           // threads of every workgroup here
static constexpr int PDQ_PLANES = 5;                         // pPDQ, Q_S, Q_L, L_FG, L_BG
static constexpr int PDQ_INVALID = 1 << 30;                  // in a detection's row word: it matches nothing

struct PdqRecord { int32_t i[4]; double d[5]; };
static_assert(sizeof(PdqRecord) == BYOLO_PDQ_RECORD_BYTES, "include/byolo.h: BYOLO_PDQ_RECORD_BYTES");

// one image's slice of the workspace (byte offsets; every part 8-byte aligned)
struct PdqLayout {
    size_t hdr, det_row, det_par, gt_idx, gt_rect, gt_label, mat, stride;
    int nd, G;
};
static PdqLayout pdq_layout(int cap, int gmax) {
    PdqLayout l;
    l.nd = cap < PDQ_MAX_DET ? cap : PDQ_MAX_DET;
    l.G = gmax;
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o += (bytes + 7) / 8 * 8; return at; };
    l.hdr = take(4 * sizeof(int32_t));                       // n_det, n_gt, flags, 0
    l.det_row = take((size_t)l.nd * sizeof(int32_t));
    l.det_par = take((size_t)l.nd * 6 * sizeof(double));     // X0, X1, Y0, Y1, sx, sy
    l.gt_idx = take((size_t)l.G * sizeof(int32_t));
    l.gt_rect = take((size_t)l.G * 4 * sizeof(int32_t));     // u0, u1, v0, v1
    l.gt_label = take((size_t)l.G * sizeof(int32_t));
    l.mat = take((size_t)PDQ_PLANES * l.nd * l.G * sizeof(double));
    l.stride = o;
    return l;
}
size_t pdq_workspace_bytes(int B, int cap, int gmax) {
    if (B < 1 || B > 65535 || cap < 1 || cap > 4096 || gmax < 1 || gmax > BYOLO_EVAL_MAX_GT) return 0;
    return pdq_layout(cap, gmax).stride * (size_t)B;
}

struct PdqArgs {
    PdqBatch b;
    char* ws;
    PdqLayout l;
    int32_t var, ale_col, epi_col, img_h, img_w;
    float min_score;
    double p_min, eps, var_floor;
    int32_t layer_col, prior_col, n_layers;
    int32_t lh[BYOLO_EVAL_LOC_MAX_LAYERS], lw[BYOLO_EVAL_LOC_MAX_LAYERS], n_priors[BYOLO_EVAL_LOC_MAX_LAYERS];
    PdqRecord* images; PdqRecord* pairs;
    long long image_cap, pair_cap;
    int32_t* state;
};

__device__ __forceinline__ int pdq_clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ bool pdq_finite(float v) { return fabsf(v) <= FLT_MAX; }          // false for NaN and inf

// the main table's rule: class = first index of the largest class score, score = obj * cls[class] in one float32 multiply; a NaN
// class score drops the row.  Here the score must also be finite
__device__ __forceinline__ bool pdq_score(const float* r, const PdqArgs& a, float& score) {
    float best = r[a.b.cls_start];
    bool nan = best != best;
    for (int c = 1; c < a.b.C; ++c) {
        const float v = r[a.b.cls_start + c];
        nan |= v != v;
        if (v > best) best = v;
    }
    score = __fmul_rn(r[a.b.obj_idx], best);
    return !nan && score >= a.min_score && pdq_finite(score);
}

__device__ __forceinline__ void pdq_ce(unsigned long long& x, unsigned long long& y, bool up) {
    if ((x > y) == up) { const unsigned long long t = x; x = y; y = t; }
}

__device__ __forceinline__ bool pdq_id(float v, int n, int& out) {      // finite, integral, inside [0, n)
    const bool ok = v >= 0.f && v < (float)n && floorf(v) == v;
    out = ok ? (int)v : 0;
    return ok;
}
__device__ __forceinline__ bool pdq_var(const float* r, const PdqArgs& a, int c, double& v) {
    bool ok = true;
    v = 0.0;
    if (a.var == BYOLO_VOTE_ALE || a.var == BYOLO_VOTE_TOTAL) { const float x = r[a.ale_col + c]; ok = ok && pdq_finite(x) && x >= 0.f; v += (double)x; }
    if (a.var == BYOLO_VOTE_EPI || a.var == BYOLO_VOTE_TOTAL) { const float x = r[a.epi_col + c]; ok = ok && pdq_finite(x) && x >= 0.f; v += (double)x; }
    return ok;
}
// position of a centre inside its cell, as the variance voting takes it
__device__ __forceinline__ double pdq_frac(double c, int n) {
    const double s = c * (double)n;
    double f = floor(s);
    f = f < 0.0 ? 0.0 : (f > (double)(n - 1) ? (double)(n - 1) : f);
    const double q = s - f;
    return q < 0.0 ? 0.0 : (q > 1.0 ? 1.0 : q);
}
// first pixel whose centre is not left of X, clipped to [0, n]
__device__ __forceinline__ int pdq_edge(double X, int n) {
    double e = ceil(X - 0.5);
    e = e < 0.0 ? 0.0 : (e > (double)n ? (double)n : e);
    return (int)e;
}

__global__ __launch_bounds__(PDQ_NT) void pdq_list_kernel(const PdqArgs a) {
    __shared__ unsigned long long key[PDQ_MAX_DET];
    __shared__ int s_ns, s_wcnt[PDQ_NT / 64];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    char* img = a.ws + (size_t)b * a.l.stride;
    int32_t* hdr = reinterpret_cast<int32_t*>(img + a.l.hdr);
    int32_t* det_row = reinterpret_cast<int32_t*>(img + a.l.det_row);
    double* det_par = reinterpret_cast<double*>(img + a.l.det_par);
    int32_t* gt_idx = reinterpret_cast<int32_t*>(img + a.l.gt_idx);
    int32_t* gt_rect = reinterpret_cast<int32_t*>(img + a.l.gt_rect);
    int32_t* gt_label = reinterpret_cast<int32_t*>(img + a.l.gt_label);
    if (tid == 0) s_ns = 0;
    __syncthreads();

    // the detections: keys of the eligible rows
    const int n = pdq_clampi(a.b.count[(size_t)b * a.b.count_stride], 0, a.b.cap);
    const float* rows = a.b.rows + (size_t)b * a.b.cap * a.b.D;
    for (int i0 = 0; i0 < n; i0 += PDQ_NT) {
        const int i = i0 + tid;
        float s = 0.f;
        const bool ok = i < n && pdq_score(rows + (size_t)i * a.b.D, a, s);
        const unsigned long long m = __ballot(ok);
        int at = 0;
        if (lane == 0 && m) at = atomicAdd(&s_ns, __popcll(m));      // LDS
        at = __shfl(at, 0);
        const int slot = at + __popcll(m & ((1ull << lane) - 1ull));
        // nms_box.h's key: ascending key = descending score, either zero the key of +0
        if (ok && slot < PDQ_MAX_DET) key[slot] = ((unsigned long long)score_key(s) << 32) | (unsigned int)i;
    }
    __syncthreads();
    int ns = s_ns, flags = 0;
    if (ns > PDQ_MAX_DET) {                                  // never a silent cut: the image is not evaluated and finish fails
        ns = 0; flags = 1;
        if (tid == 0) atomicOr(&a.state[PDQ_ST_FLAGS], (int)PDQ_FLAG_DET);
    }
    int P2 = 64;
    while (P2 < ns) P2 <<= 1;
    __syncthreads();
    for (int i = ns + tid; i < P2; i += PDQ_NT) key[i] = ~0ull;
    __syncthreads();
    for (int k = 2; k <= P2; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < P2 / 2; t += PDQ_NT) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                pdq_ce(key[i], key[i + j], (i & k) == 0);
            }
            __syncthreads();
        }

    // the corner distributions
    const double W = (double)a.img_w, H = (double)a.img_h;
    for (int d = tid; d < ns; d += PDQ_NT) {
        const int row = (int)(key[d] & 0xffffffffull);
        const float* r = rows + (size_t)row * a.b.D;
        const float b0 = r[0], b1 = r[1], b2 = r[2], b3 = r[3];
        const NBox bx = make_box(b0, b1, b2, b3);
        bool ok = pdq_finite(b0) && pdq_finite(b1) && pdq_finite(b2) && pdq_finite(b3);
        double var_x = 0.0, var_y = 0.0, var_w = 0.0, var_h = 0.0;
        if (ok && a.var != BYOLO_VOTE_NONE) {
            int layer = 0, prior = 0;
            ok = pdq_id(r[a.layer_col], a.n_layers, layer);
            if (ok) ok = pdq_id(r[a.prior_col], a.n_priors[layer], prior);
            double vx, vy, vw, vh;
            ok = pdq_var(r, a, 0, vx) && ok; ok = pdq_var(r, a, 1, vy) && ok; ok = pdq_var(r, a, 2, vw) && ok; ok = pdq_var(r, a, 3, vh) && ok;
            if (ok) {
                const int lh = a.lh[layer], lw = a.lw[layer];
                const double cx = ((double)bx.x0 + (double)bx.x1) * 0.5, cy = ((double)bx.y0 + (double)bx.y1) * 0.5;
                const double bw = (double)bx.x1 - (double)bx.x0, bh = (double)bx.y1 - (double)bx.y0;
                const double fx = pdq_frac(cx, lw), fy = pdq_frac(cy, lh);
                const double tx = fx * (1.0 - fx) / (double)lw, ty = fy * (1.0 - fy) / (double)lh;
                var_x = vx * (tx * tx); var_y = vy * (ty * ty);
                var_w = vw * (bw * bw); var_h = vh * (bh * bh);
            }
        }
        double* p = det_par + (size_t)d * 6;
        p[0] = (double)bx.x0 * W; p[1] = (double)bx.x1 * W; p[2] = (double)bx.y0 * H; p[3] = (double)bx.y1 * H;
        p[4] = sqrt(fmax((var_x + var_w / 4.0) * (W * W), a.var_floor));
        p[5] = sqrt(fmax((var_y + var_h / 4.0) * (H * H), a.var_floor));
        det_row[d] = ok ? row : (row | PDQ_INVALID);
    }

    // the counted boxes, compacted in ascending index
    const int G = pdq_clampi(a.b.gt_counts[b], 0, a.b.gmax);
    int done = 0;
    for (int g0 = 0; g0 < G; g0 += PDQ_NT) {
        const int g = g0 + tid;
        bool cnt = false;
        int u0 = 0, u1 = 0, v0 = 0, v1 = 0, lab = -1;
        if (g < G) {
            const float* q = a.b.gt_boxes + ((size_t)b * a.b.gmax + g) * 4;
            const float q0 = q[0], q1 = q[1], q2 = q[2], q3 = q[3];
            lab = a.b.gt_labels[(size_t)b * a.b.gmax + g];
            if (lab >= 0 && lab < a.b.C && pdq_finite(q0) && pdq_finite(q1) && pdq_finite(q2) && pdq_finite(q3)) {
                const NBox o = make_box(q0, q1, q2, q3);
                u0 = pdq_edge((double)o.x0 * W, a.img_w); u1 = pdq_edge((double)o.x1 * W, a.img_w);
                v0 = pdq_edge((double)o.y0 * H, a.img_h); v1 = pdq_edge((double)o.y1 * H, a.img_h);
                cnt = u1 > u0 && v1 > v0;
            }
        }
        const unsigned long long m = __ballot(cnt);
        if (lane == 0) s_wcnt[wave] = __popcll(m);
        __syncthreads();
        int at = done, all = 0;
        for (int w = 0; w < PDQ_NT / 64; ++w) { if (w < wave) at += s_wcnt[w]; all += s_wcnt[w]; }
        at += __popcll(m & ((1ull << lane) - 1ull));
        if (cnt) {
            gt_idx[at] = g; gt_label[at] = lab;
            gt_rect[4 * at + 0] = u0; gt_rect[4 * at + 1] = u1; gt_rect[4 * at + 2] = v0; gt_rect[4 * at + 3] = v1;
        }
        done += all;
        __syncthreads();
    }
    if (tid == 0) { hdr[0] = ns; hdr[1] = done; hdr[2] = flags; hdr[3] = 0; }
}

// ---- the pairs ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double pdq_phi(double z) { return 0.5 * erfc(-z / 1.4142135623730951); }

// the workgroup's sum in a fixed order; red: PDQ_NT / 64 doubles of LDS.  Every thread gets the result
__device__ __forceinline__ double pdq_block_sum(double v, double* red, int tid) {
#pragma unroll
    for (int sft = 1; sft < 64; sft <<= 1) v += __shfl_xor(v, sft);
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    const double r = ((red[0] + red[1]) + red[2]) + red[3];
    __syncthreads();
    return r;
}
static_assert(PDQ_NT == 256, "pdq_block_sum folds four waves");

__global__ __launch_bounds__(PDQ_NT) void pdq_pair_kernel(const PdqArgs a) {
    extern __shared__ double s_p[];                          // px[img_w], py[img_h]
    __shared__ double s_red[PDQ_NT / 64];
    __shared__ int s_box[4];                                 // the support: u0, u1 - 1, v0, v1 - 1
    const int b = blockIdx.y, d = blockIdx.x, tid = threadIdx.x;
    const char* img = a.ws + (size_t)b * a.l.stride;
    const int32_t* hdr = reinterpret_cast<const int32_t*>(img + a.l.hdr);
    const int n_det = hdr[0], n_gt = hdr[1];
    if (d >= n_det || n_gt == 0) return;
    const int32_t* gt_rect = reinterpret_cast<const int32_t*>(img + a.l.gt_rect);
    const int32_t* gt_label = reinterpret_cast<const int32_t*>(img + a.l.gt_label);
    double* mat = reinterpret_cast<double*>(const_cast<char*>(img) + a.l.mat);
    const size_t plane = (size_t)a.l.nd * a.l.G;
    double* out = mat + (size_t)d * a.l.G;
    const int W = a.img_w, H = a.img_h;
    double* px = s_p;
    double* py = s_p + W;
    const int row_word = reinterpret_cast<const int32_t*>(img + a.l.det_row)[d];
    const bool valid = !(row_word & PDQ_INVALID);
    const float* r = a.b.rows + ((size_t)b * a.b.cap + (row_word & ~PDQ_INVALID)) * a.b.D;

    if (tid == 0) { s_box[0] = W; s_box[1] = -1; s_box[2] = H; s_box[3] = -1; }
    __syncthreads();
    if (valid) {
        const double* p = reinterpret_cast<const double*>(img + a.l.det_par) + (size_t)d * 6;
        const double X0 = p[0], X1 = p[1], Y0 = p[2], Y1 = p[3], sx = p[4], sy = p[5];
        for (int u = tid; u < W; u += PDQ_NT) {
            const double v = pdq_phi((((double)u + 0.5) - X0) / sx) * pdq_phi(((X1 - (double)u) - 0.5) / sx);
            px[u] = v;
            if (v >= a.p_min) { atomicMin(&s_box[0], u); atomicMax(&s_box[1], u); }
        }
        for (int v = tid; v < H; v += PDQ_NT) {
            const double q = pdq_phi((((double)v + 0.5) - Y0) / sy) * pdq_phi(((Y1 - (double)v) - 0.5) / sy);
            py[v] = q;
            if (q >= a.p_min) { atomicMin(&s_box[2], v); atomicMax(&s_box[3], v); }
        }
    }
    __syncthreads();
    const int ru0 = s_box[0], ru1 = s_box[1] + 1, rv0 = s_box[2], rv1 = s_box[3] + 1;
    const bool support = valid && ru1 > ru0 && rv1 > rv0;
    const double log_eps = log(a.eps);
    const float obj = r[a.b.obj_idx];

    for (int c = 0; c < n_gt; ++c) {                         // every branch below is uniform over the workgroup
        const int gu0 = gt_rect[4 * c + 0], gu1 = gt_rect[4 * c + 1], gv0 = gt_rect[4 * c + 2], gv1 = gt_rect[4 * c + 3];
        const int iu0 = max(gu0, ru0), iu1 = min(gu1, ru1), iv0 = max(gv0, rv0), iv1 = min(gv1, rv1);
        double ppdq = 0.0, qs = 0.0, ql = 0.0, lfg = 0.0, lbg = 0.0;
        if (support && iu1 > iu0 && iv1 > iv0) {
            // the box inside the support
            const int wi = iu1 - iu0, n_in = wi * (iv1 - iv0);
            double acc = 0.0, hit = 0.0;
            for (int k = tid; k < n_in; k += PDQ_NT) {
                const int v = iv0 + k / wi, u = iu0 + k % wi;
                const double p = px[u] * py[v];
                if (p >= a.p_min) { acc += log(fmax(p, a.eps)); hit += 1.0; }
                else acc += log_eps;
            }
            const double hits = pdq_block_sum(hit, s_red, tid);
            if (hits > 0.0) {                                // a shared pixel
                const double area = (double)(gu1 - gu0) * (double)(gv1 - gv0);
                const double fg = pdq_block_sum(acc, s_red, tid) + (area - (double)n_in) * log_eps;
                // the support without the box
                const int wr = ru1 - ru0, n_r = wr * (rv1 - rv0);
                acc = 0.0;
                for (int k = tid; k < n_r; k += PDQ_NT) {
                    const int v = rv0 + k / wr, u = ru0 + k % wr;
                    if (u >= gu0 && u < gu1 && v >= gv0 && v < gv1) continue;
                    const double p = px[u] * py[v];
                    if (p >= a.p_min) acc += log(fmax(1.0 - p, a.eps));
                }
                const double bg = pdq_block_sum(acc, s_red, tid);
                lfg = -(fg / area);
                lbg = -(bg / area);
                qs = exp(-(lfg + lbg));
                ql = (double)__fmul_rn(obj, r[a.b.cls_start + gt_label[c]]);
                if (!(ql >= 0.0)) ql = 0.0;                  // NaN too
                if (ql > 1.0) ql = 1.0;
                ppdq = sqrt(qs * ql);
            }
        }
        if (tid == 0) {
            out[c] = ppdq; out[plane + c] = qs; out[2 * plane + c] = ql; out[3 * plane + c] = lfg; out[4 * plane + c] = lbg;
        }
    }
}

// ---- the assignment ------------------------------------------------------------------------------------------------------------
struct AssignLds {
    double u[PDQ_MAX_DET + 1], v[PDQ_MAX_DET + 1], minv[PDQ_MAX_DET + 1];
    int p[PDQ_MAX_DET + 1], way[PDQ_MAX_DET + 1], used[PDQ_MAX_DET + 1];
    double rv[PDQ_NT / 64];
    int rj[PDQ_NT / 64];
};

// smaller value, then lower column
__device__ __forceinline__ void pdq_argmin(double& bv, int& bj, double ov, int oj) {
    if (ov < bv || (ov == bv && oj < bj)) { bv = ov; bj = oj; }
}

// rows 1 .. n against columns 1 .. m (n <= m <= PDQ_MAX_DET) of cost[i][j] = -M[(i - 1) * rs + (j - 1) * cs]; leaves L.p[j] = the
// row of column j, or 0.  Every thread of the workgroup calls it.  The entries must be finite: the pair kernel's are; on anything
// else the search stops where no column can be reached and leaves the matching it has
__device__ void pdq_hungarian(const double* M, size_t rs, size_t cs, int n, int m, AssignLds& L, int tid) {
    const double INF = __longlong_as_double(0x7ff0000000000000ll);
    for (int j = tid; j <= m; j += PDQ_NT) { L.v[j] = 0.0; L.p[j] = 0; L.way[j] = 0; }
    for (int i = tid; i <= n; i += PDQ_NT) L.u[i] = 0.0;
    __syncthreads();
    for (int i = 1; i <= n; ++i) {
        for (int j = tid; j <= m; j += PDQ_NT) { L.minv[j] = INF; L.used[j] = 0; }
        if (tid == 0) L.p[0] = i;
        int j0 = 0;
        while (true) {
            __syncthreads();
            if (tid == 0) L.used[j0] = 1;
            __syncthreads();
            const int i0 = L.p[j0];
            const double ui0 = L.u[i0];
            double best = INF;
            int bj = 0x7fffffff;
            for (int j = tid + 1; j <= m; j += PDQ_NT) {
                if (L.used[j]) continue;
                const double cost = -M[(size_t)(i0 - 1) * rs + (size_t)(j - 1) * cs];
                const double cur = (cost - ui0) - L.v[j];
                double mv = L.minv[j];
                if (cur < mv) { mv = cur; L.minv[j] = cur; L.way[j] = j0; }
                if (mv < best) { best = mv; bj = j; }
            }
#pragma unroll
            for (int sft = 1; sft < 64; sft <<= 1) pdq_argmin(best, bj, __shfl_xor(best, sft), __shfl_xor(bj, sft));
            if ((tid & 63) == 0) { L.rv[tid >> 6] = best; L.rj[tid >> 6] = bj; }
            __syncthreads();
            double delta = L.rv[0];
            int j1 = L.rj[0];
#pragma unroll
            for (int w = 1; w < PDQ_NT / 64; ++w) pdq_argmin(delta, j1, L.rv[w], L.rj[w]);
            if (j1 == 0x7fffffff) return;                    // no free column has a finite distance: the matrix holds NaN or inf (uniform)
            for (int j = tid; j <= m; j += PDQ_NT) {
                if (L.used[j]) { L.u[L.p[j]] += delta; L.v[j] -= delta; }
                else L.minv[j] -= delta;
            }
            j0 = j1;
            __syncthreads();
            if (L.p[j0] == 0) break;                         // uniform: p is not written inside this loop
        }
        __syncthreads();                                     // every thread has read p[j0] before the path is flipped
        if (tid == 0) {
            do { const int j1 = L.way[j0]; L.p[j0] = L.p[j1]; j0 = j1; } while (j0);
        }
        __syncthreads();
    }
}

// the matching of an [n_det, n_gt] matrix with row stride `stride`: L.way[d] = the column of detection d, or -1
__device__ void pdq_match(const double* M, size_t stride, int n_det, int n_gt, AssignLds& L, int tid) {
    const bool det_rows = n_det <= n_gt;                     // the smaller side is the rows; equal: the detections
    const int n = det_rows ? n_det : n_gt, m = det_rows ? n_gt : n_det;
    if (n > 0) pdq_hungarian(M, det_rows ? stride : 1, det_rows ? 1 : stride, n, m, L, tid);
    __syncthreads();
    for (int d = tid; d < n_det; d += PDQ_NT) L.way[d + 1] = -1;        // way has done its work: slot d + 1 is detection d
    __syncthreads();
    if (n > 0)
        for (int j = tid + 1; j <= m; j += PDQ_NT) {
            const int i = L.p[j];
            if (det_rows) { if (i) L.way[i] = j - 1; }
            else L.way[j] = i - 1;
        }
    __syncthreads();
}

__global__ __launch_bounds__(PDQ_NT) void pdq_assign_kernel(const PdqArgs a) {
    __shared__ AssignLds L;
    const int b = blockIdx.x, tid = threadIdx.x;
    const char* img = a.ws + (size_t)b * a.l.stride;
    const int32_t* hdr = reinterpret_cast<const int32_t*>(img + a.l.hdr);
    const int n_det = hdr[0], n_gt = hdr[1], flags = hdr[2];
    const int32_t* det_row = reinterpret_cast<const int32_t*>(img + a.l.det_row);
    const int32_t* gt_idx = reinterpret_cast<const int32_t*>(img + a.l.gt_idx);
    const double* mat = reinterpret_cast<const double*>(img + a.l.mat);
    const size_t plane = (size_t)a.l.nd * a.l.G;
    pdq_match(mat, (size_t)a.l.G, n_det, n_gt, L, tid);
    if (tid != 0) return;
    // the records: one thread, ascending detection -- the order of the sums
    PdqRecord rec;
    rec.i[0] = n_det; rec.i[1] = n_gt; rec.i[3] = flags;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0, s4 = 0.0;
    int n_tp = 0;
    if (n_gt > 0)
        for (int d = 0; d < n_det; ++d) {
            const int c = L.way[d + 1];
            if (c < 0) continue;
            const double* e = mat + (size_t)d * a.l.G + c;
            if (!(e[0] > 0.0)) continue;
            s0 += e[0]; s1 += e[plane]; s2 += e[2 * plane]; s3 += exp(-e[3 * plane]); s4 += exp(-e[4 * plane]);
            ++n_tp;
        }
    rec.i[2] = n_tp;
    rec.d[0] = s0; rec.d[1] = s1; rec.d[2] = s2; rec.d[3] = s3; rec.d[4] = s4;
    const long long at_img = (long long)a.b.img_base + b;
    if (at_img < a.image_cap) a.images[at_img] = rec;
    else atomicOr(&a.state[PDQ_ST_FLAGS], (int)PDQ_FLAG_IMAGES);
    if (n_tp == 0) return;
    long long at = (long long)atomicAdd(reinterpret_cast<unsigned long long*>(a.state + PDQ_ST_CURSOR), (unsigned long long)n_tp);
    if (at + n_tp > a.pair_cap) atomicOr(&a.state[PDQ_ST_FLAGS], (int)PDQ_FLAG_PAIRS);
    for (int d = 0; d < n_det; ++d) {
        const int c = L.way[d + 1];
        if (c < 0) continue;
        const double* e = mat + (size_t)d * a.l.G + c;
        if (!(e[0] > 0.0)) continue;
        if (at < a.pair_cap) {
            PdqRecord pr;
            pr.i[0] = (int32_t)at_img; pr.i[1] = det_row[d] & ~PDQ_INVALID; pr.i[2] = gt_idx[c]; pr.i[3] = 0;
            pr.d[0] = e[0]; pr.d[1] = e[plane]; pr.d[2] = e[2 * plane]; pr.d[3] = e[3 * plane]; pr.d[4] = e[4 * plane];
            a.pairs[at] = pr;
        }
        ++at;
    }
}

// byolo_pdq_assign: the stage alone
__global__ __launch_bounds__(PDQ_NT) void pdq_assign_alone_kernel(const double* M, int n_det, int n_gt, int32_t* out) {
    __shared__ AssignLds L;
    const int tid = threadIdx.x;
    pdq_match(M, (size_t)n_gt, n_det, n_gt, L, tid);
    for (int d = tid; d < n_det; d += PDQ_NT) out[d] = L.way[d + 1];
}

const char* pdq_check(const byolo_eval_pdq_cfg* c, const byolo_eval_loc_cfg* g, int D) {
    if (c->var < BYOLO_VOTE_NONE || c->var > BYOLO_VOTE_TOTAL) return "unknown var (BYOLO_VOTE_*)";
    const bool ale = c->var == BYOLO_VOTE_ALE || c->var == BYOLO_VOTE_TOTAL, epi = c->var == BYOLO_VOTE_EPI || c->var == BYOLO_VOTE_TOTAL;
    if (ale && c->ale_col < 0) return "var needs aleatoric variances, these rows have none (ale_col)";
    if (epi && c->epi_col < 0) return "var needs epistemic variances, these rows have none (epi_col)";
    if (ale && (int64_t)c->ale_col + 4 > D) return "ale_col .. +3 outside the row";
    if (epi && (int64_t)c->epi_col + 4 > D) return "epi_col .. +3 outside the row";
    if (c->min_score != c->min_score) return "min_score is NaN";
    if (!(c->p_min > 0.0 && c->p_min < 1.0)) return "p_min outside (0, 1)";
    if (!(c->eps > 0.0 && c->eps <= c->p_min)) return "eps outside (0, p_min]";
    if (!(c->var_floor > 0.0 && c->var_floor <= DBL_MAX)) return "var_floor is not finite and > 0";
    if (c->img_h < 1 || c->img_h > BYOLO_PDQ_MAX_FRAME || c->img_w < 1 || c->img_w > BYOLO_PDQ_MAX_FRAME) return "img_h / img_w outside 1 .. 4096";
    if (c->var != BYOLO_VOTE_NONE) {
        if (!g) return "geom is NULL (only BYOLO_VOTE_NONE goes without the geometry table)";
        if (g->struct_bytes != (int32_t)sizeof *g) return "geom->struct_bytes is not this library's sizeof(byolo_eval_loc_cfg)";
        if (g->layer_col < 0 || g->layer_col >= D || g->prior_col < 0 || g->prior_col >= D) return "geom: layer_col / prior_col outside the row";
        if (g->n_layers < 1 || g->n_layers > BYOLO_EVAL_LOC_MAX_LAYERS) return "geom->n_layers outside its limits";
        for (int l = 0; l < g->n_layers; ++l) {
            if (g->n_priors[l] < 1 || g->n_priors[l] > BYOLO_EVAL_LOC_MAX_PRIORS) return "geom->n_priors outside its limits";
            if (g->lh[l] < 1 || g->lw[l] < 1) return "geom: a grid below 1 x 1";
        }
    }
    return nullptr;
}

hipError_t pdq_fetch_matrix(const PdqSide& s, int cap, int gmax, int image, int32_t* h_counts, int32_t* h_rows, int32_t* h_gts, double* h_planes,
                            hipStream_t st) {
    const PdqLayout l = pdq_layout(cap, gmax);
    const char* img = static_cast<const char*>(s.d_ws) + (size_t)image * l.stride;
    int32_t hdr[4];
    hipError_t e = hipMemcpyAsync(hdr, img + l.hdr, sizeof hdr, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(h_rows, img + l.det_row, sizeof(int32_t) * (size_t)l.nd, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(h_gts, img + l.gt_idx, sizeof(int32_t) * (size_t)l.G, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(h_planes, img + l.mat, sizeof(double) * PDQ_PLANES * (size_t)l.nd * l.G, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return e;
    h_counts[0] = hdr[0]; h_counts[1] = hdr[1];
    for (int d = 0; d < l.nd; ++d) h_rows[d] &= ~PDQ_INVALID;
    return hipSuccess;
}

// dynamic LDS of pdq_pair_kernel: px and py of the frame (the kernel has 48 bytes of static LDS besides)
static size_t pdq_pair_lds(const byolo_eval_pdq_cfg& c) { return sizeof(double) * ((size_t)c.img_w + (size_t)c.img_h); }

// byolo_eval_set_pdq: whatever can fail for these settings fails here, before a batch is half launched
hipError_t pdq_prepare(const byolo_eval_pdq_cfg& c) {
    const size_t lds = pdq_pair_lds(c);
    if (lds <= 48 * 1024) return hipSuccess;                 // within what any launch may ask for
    return hipFuncSetAttribute(reinterpret_cast<const void*>(pdq_pair_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
}

hipError_t pdq_launch(const PdqSide& s, const PdqBatch& b, hipStream_t st) {
    PdqArgs a;
    memset(&a, 0, sizeof a);
    a.b = b;
    a.ws = static_cast<char*>(s.d_ws);
    a.l = pdq_layout(b.cap, b.gmax);
    if (a.l.stride * (size_t)b.B > s.ws_bytes) return hipErrorInvalidValue;      // byolo_eval_add has refused it already
    a.var = s.cfg.var; a.ale_col = s.cfg.ale_col; a.epi_col = s.cfg.epi_col; a.img_h = s.cfg.img_h; a.img_w = s.cfg.img_w;
    a.min_score = s.cfg.min_score; a.p_min = s.cfg.p_min; a.eps = s.cfg.eps; a.var_floor = s.cfg.var_floor;
    if (s.cfg.var != BYOLO_VOTE_NONE) {
        a.layer_col = s.geom.layer_col; a.prior_col = s.geom.prior_col; a.n_layers = s.geom.n_layers;
        for (int l = 0; l < s.geom.n_layers; ++l) { a.lh[l] = s.geom.lh[l]; a.lw[l] = s.geom.lw[l]; a.n_priors[l] = s.geom.n_priors[l]; }
    }
    a.images = static_cast<PdqRecord*>(s.d_images); a.pairs = static_cast<PdqRecord*>(s.d_pairs);
    a.image_cap = s.image_capacity; a.pair_cap = s.pair_capacity;
    a.state = static_cast<int32_t*>(s.d_state);
    const size_t lds = pdq_pair_lds(s.cfg);                  // pdq_prepare has raised the kernel's limit where that is needed
    hipLaunchKernelGGL(pdq_list_kernel, dim3(b.B), dim3(PDQ_NT), 0, st, a);
    hipLaunchKernelGGL(pdq_pair_kernel, dim3(a.l.nd, b.B), dim3(PDQ_NT), lds, st, a);
    hipLaunchKernelGGL(pdq_assign_kernel, dim3(b.B), dim3(PDQ_NT), 0, st, a);
    return hipGetLastError();
}

}  // namespace byk

extern "C" size_t byolo_eval_pdq_workspace_bytes(int32_t B, int32_t cap, int32_t gmax) { return byk::pdq_workspace_bytes(B, cap, gmax); }

extern "C" size_t byolo_eval_pdq_state_bytes(void) { return sizeof(int32_t) * byk::PDQ_ST_WORDS; }

extern "C" int32_t byolo_pdq_assign(const double* d_matrix, int32_t n_det, int32_t n_gt, int32_t* d_out_match, void* stream) {
    if (n_det < 0 || n_det > BYOLO_PDQ_MAX_DET || n_gt < 0 || n_gt > BYOLO_PDQ_MAX_DET)
        return byk::efail(nullptr, BYOLO_ERR_ARG, "byolo_pdq_assign: n_det / n_gt outside 0 .. %d", BYOLO_PDQ_MAX_DET);
    if (n_det == 0) return BYOLO_OK;
    if (!d_out_match || (n_gt > 0 && !d_matrix)) return byk::efail(nullptr, BYOLO_ERR_ARG, "byolo_pdq_assign: null argument");
    if ((reinterpret_cast<uintptr_t>(d_matrix) & 7) || (reinterpret_cast<uintptr_t>(d_out_match) & 3))
        return byk::efail(nullptr, BYOLO_ERR_ARG, "byolo_pdq_assign: d_matrix must be 8-byte and d_out_match 4-byte aligned");
    hipLaunchKernelGGL(byk::pdq_assign_alone_kernel, dim3(1), dim3(byk::PDQ_NT), 0, static_cast<hipStream_t>(stream), d_matrix, n_det, n_gt, d_out_match);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return byk::efail(nullptr, BYOLO_ERR_HIP, "byolo_pdq_assign: launch failed: %s", hipGetErrorString(e));
    return BYOLO_OK;
}
