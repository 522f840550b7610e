// eval_kernels.hip -- scoring a checkpoint on labelled frames (include/byolo.h byolo_eval_*): the kept rows of a batch
// (byolo_sort_nms) are matched against the frames' ground truth on the forward's stream, one launch per batch, and appended
// as records to a device-resident table.  No allocation, no host wait: the running record offset, the per-class ground-truth
// counters and the image counter live in a small device state that only byolo_eval_finish reads back.
//
// Matching is the Dollar / ECP / COCO rule: per image, detections in descending score (ties: lower row), each takes the
// not-yet-matched ground-truth box OF ITS CLASS with the largest IoU (ties: lower box index); a true positive iff that IoU
// >= iou_thresh, and only then is the box marked.  IoU is nms_box.h's: the float32 operations of the NMS, in the same order.
//
// The matching of one image is written once, as stages over the (tid, nthreads) of the image's workgroup:
//   1  the image's ground truth -> LDS as NBox + label (label outside [0, C) = not eligible)
//   2  rows -> (score, row, class) keys of the surviving rows in LDS: the waves take turns at 64 rows, an LDS counter hands each
//      ballot its slots; class = first index of the largest class score, score = obj * cls[class] (one float32 multiply),
//      dropped when NaN or below min_score.  The keys are distinct, so their order before the sort does not matter
//   3  where the image's records start: the device's running offset + the survivors of the images before it in the batch,
//      which every workgroup counts for itself, each wave a share summed through LDS (a few thousand rows; cheaper than a
//      second launch or a wait between workgroups)
//   4  bitonic sort of the keys (LDS)
//   5  the greedy pass of ONE wave at one threshold: 64 detections per round, one per lane (box and class in registers); the
//      round walks them in order: the detection is broadcast, every lane scores the ground-truth boxes lane, lane + 64, ...
//      against it, a cross-lane arg-max picks the box; the matched set is one bit per pass in a per-lane word
//   6  the writer, which is what the two kernels below differ in
// Float arithmetic here is restated operation by operation (tests/_eval_ref.py): built with -ffp-contract=off.
//
// eval_match_kernel: one wave64 per image, the threshold is the evaluator's iou_thresh.  Stage 1 also adds the eligible boxes to
// the class counters and the image to the image counter, the last image of the launch leaves the next launch's offset behind
// stage 3, and every lane writes its detection's record with the uncertainty columns; a record beyond the capacity sets the
// sticky overflow word instead.
//
// eval_ladder_kernel (byolo_eval_set_ladder): behind the match kernel on the same stream, one workgroup per image and one wave64
// per threshold.  The matching depends on the threshold (a box a detection fails to claim stays open for a later one), so every
// threshold gets the pass of stage 5 of its own, with its own matched set; stages 1 - 4 are run ONCE by all waves together, and
// stage 3 arrives at the start the match kernel used (the running offset this launch reads is the word the match kernel does
// not write).  The true-positive bits of a detection meet in the upper half of its sorted key, which the passes no longer read;
// the records go to a third table, 1 + n_thr words each, at the record's own index.  Neither the main table nor the device
// state is written.
//
// eval_subset_kernel (byolo_eval_set_subsets): behind the match kernel on the same stream, one workgroup per image and one wave64
// per subset of the ground truth by pixel height -- the protocol of the pedestrian benchmarks.  Stages 1 - 4 as the ladder runs
// them; stage 5 is a pass of its own (ev_subset_pass) in which a detection that finds no counted box may be excused by an ignore
// region or by its own height.  The 2-bit states of a detection meet in the upper half of its sorted key; the records go to a
// fourth table, 1 + n_subsets words each, and the counted boxes per (subset, class) to a state buffer of the table's own.
//
// eval_loc_kernel (byolo_eval_set_loc): right behind the match kernel on the same stream, one thread per record of the launch.
// A true positive's box and its matched ground-truth box are taken back to the raw location values t_x, t_y, t_w, t_h at the
// detection's own cell and prior (the row's layer_id / prior_id columns), in float64, one operation per line as
// tests/_eval_loc_ref.py restates them; the residuals t(ground truth) - t(detection) go to a second table, six words per record.
//
// Probabilistic detection quality (byolo_eval_set_pdq): its three kernels live in eval_pdq.hip and follow the launches above on the
// same stream; they read the rows and the ground truth, not the tables here.  This file keeps the handle and the C-ABI around them.
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <new>
#include <string>

#include "../../include/byolo.h"
#include "eval_pdq.h"
#include "nms_box.h"

namespace byk {

static constexpr int EV_MAX_DET = 4096;                      // rows per image (cap): the keys of one image sort in LDS
static constexpr int EV_MAX_GT = BYOLO_EVAL_MAX_GT;          // ground-truth boxes per image staged in LDS
static constexpr int EV_HEAD = BYOLO_EVAL_RECORD_HEAD;       // record words before the uncertainty columns
static constexpr int EV_MAX_UNC = BYOLO_EVAL_MAX_UNC;
static constexpr int LAD_MAX = BYOLO_EVAL_LADDER_MAX;        // thresholds of a ladder = waves of its workgroup
// device state (int32 words): the running record offset twice (a launch reads one and its last image writes the other: the
// images of a launch run concurrently), the sticky overflow word, the image counter, then one counter per class
enum { ST_TOTAL0 = 0, ST_TOTAL1 = 1, ST_OVERFLOW = 2, ST_IMAGES = 3, ST_CLASS0 = 8 };

struct EvalArgs {
    const float* rows; const int32_t* count; int64_t count_stride;
    const float* gt_boxes; const int32_t* gt_labels; const int32_t* gt_counts;
    int32_t* table; int32_t* state; int64_t capacity;
    int32_t B, cap, D, obj_idx, cls_start, C, gmax, n_unc, parity, img_base;
    float iou_thresh, min_score;
    int32_t unc[EV_MAX_UNC];
};

struct EvalLds {
    unsigned long long key[EV_MAX_DET];
    float y0[EV_MAX_GT], x0[EV_MAX_GT], y1[EV_MAX_GT], x1[EV_MAX_GT], ar[EV_MAX_GT];
    int label[EV_MAX_GT];
    int part[LAD_MAX];                                       // per wave: survivors counted in the images before this one
    int ns;                                                  // the image's survivors so far: hands out the key slots
};

// what stages 1 - 4 leave for the pass and the writers, besides the LDS
struct EvalImage {
    const float* rows;
    int G, ns;                                               // ground-truth boxes staged, keys sorted
    long long base;                                          // index of the image's first record
};

// class (first index of the maximum, as np.argmax: a NaN class score wins and makes the score NaN) and score of a row;
// false: the row is dropped
__device__ __forceinline__ bool ev_score(const float* r, const EvalArgs& a, float& score, int& cls) {
    float best = r[a.cls_start];
    bool nan = best != best;
    int bi = 0;
    for (int c = 1; c < a.C; ++c) {
        const float v = r[a.cls_start + c];
        nan |= v != v;
        if (v > best) { best = v; bi = c; }
    }
    score = __fmul_rn(r[a.obj_idx], best);
    cls = bi;
    return !nan && score >= a.min_score;                     // a NaN score fails the comparison
}

__device__ __forceinline__ int ev_clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__device__ __forceinline__ void ev_ce(unsigned long long& x, unsigned long long& y, bool up) {
    if ((x > y) == up) { const unsigned long long t = x; x = y; y = t; }
}

// the halves of sorted key d (little endian): word 0 is (row << 8 | class), word 1 the score
__device__ __forceinline__ unsigned int& ev_key_word(EvalLds& L, int d, int half) {
    return reinterpret_cast<unsigned int*>(L.key)[2 * d + half];
}

// the survivors among the n rows at `rows`, 64 at a time and this wave's share of them: visit(i, ok, ballot, score, class)
template <class Visit>
__device__ __forceinline__ void ev_survivors(const float* rows, int n, const EvalArgs& a, int tid, int nthreads, Visit visit) {
    for (int i0 = tid & ~63; i0 < n; i0 += nthreads) {
        const int i = i0 + (tid & 63);
        float s = 0.f; int c = 0;
        const bool ok = i < n && ev_score(rows + (size_t)i * a.D, a, s, c);
        visit(i, ok, __ballot(ok), s, c);
    }
}

// stages 1 - 4 for image b.  MAIN: the instantiation that owns the device state's counters and the next launch's offset
template <bool MAIN>
__device__ __forceinline__ EvalImage ev_stage_and_sort(EvalLds& L, const EvalArgs& a, int b, int tid, int nthreads) {
    const int lane = tid & 63, wave = tid >> 6;
    EvalImage im;

    // 1 -- ground truth
    im.G = ev_clampi(a.gt_counts[b], 0, a.gmax);
    for (int g = tid; g < im.G; g += nthreads) {
        const float* q = a.gt_boxes + ((size_t)b * a.gmax + g) * 4;
        const NBox o = make_box(q[0], q[1], q[2], q[3]);
        int lab = a.gt_labels[(size_t)b * a.gmax + g];
        if (lab < 0 || lab >= a.C) lab = -1;
        L.y0[g] = o.y0; L.x0[g] = o.x0; L.y1[g] = o.y1; L.x1[g] = o.x1; L.ar[g] = o.area; L.label[g] = lab;
        if (MAIN && lab >= 0) atomicAdd(&a.state[ST_CLASS0 + lab], 1);
    }
    if (MAIN && tid == 0) atomicAdd(&a.state[ST_IMAGES], 1);
    if (tid == 0) L.ns = 0;
    __syncthreads();

    // 2 -- keys of the surviving rows
    const int n = ev_clampi(a.count[(size_t)b * a.count_stride], 0, a.cap);
    im.rows = a.rows + (size_t)b * a.cap * a.D;
    ev_survivors(im.rows, n, a, tid, nthreads, [&](int i, bool ok, unsigned long long m, float s, int c) {
        int at = 0;
        if (lane == 0 && m) at = atomicAdd(&L.ns, __popcll(m));  // LDS
        at = __shfl(at, 0);
        if (ok) {
            if (s == 0.f) s = 0.f;                           // -0 orders as +0
            unsigned int u = __float_as_uint(s);
            u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);  // ascending in u = ascending in s
            L.key[at + __popcll(m & ((1ull << lane) - 1ull))] = ((unsigned long long)(~u) << 32) | ((unsigned int)i << 8) | (unsigned int)c;
        }
    });

    // 3 -- survivors of the images before this one
    int part = 0;
    for (int pb = 0; pb < b; ++pb)
        ev_survivors(a.rows + (size_t)pb * a.cap * a.D, ev_clampi(a.count[(size_t)pb * a.count_stride], 0, a.cap), a, tid, nthreads,
                     [&](int, bool, unsigned long long m, float, int) { part += __popcll(m); });
    if (lane == 0) L.part[wave] = part;
    __syncthreads();
    im.ns = L.ns;
    int before = 0;
    for (int w = 0; w < (nthreads >> 6); ++w) before += L.part[w];
    im.base = (long long)a.state[ST_TOTAL0 + a.parity] + before;
    if (MAIN && b == a.B - 1 && tid == 0) {
        const long long t = im.base + im.ns;
        a.state[ST_TOTAL0 + (a.parity ^ 1)] = t > 0x7fffffffll ? 0x7fffffff : (int)t;
    }

    // 4 -- sort: descending score, then ascending row
    int P2 = 64;
    while (P2 < im.ns) P2 <<= 1;
    for (int i = im.ns + tid; i < P2; i += nthreads) L.key[i] = ~0ull;
    __syncthreads();
    for (int k = 2; k <= P2; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < P2 / 2; t += nthreads) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                ev_ce(L.key[i], L.key[i + j], (i & k) == 0);
            }
            __syncthreads();
        }
    return im;
}

// 5 -- the pass of one wave at threshold thr; every detection's lane hands write(d, row, class, its row, tp, gt, best IoU)
template <class Write>
__device__ __forceinline__ void ev_greedy_pass(EvalLds& L, const EvalArgs& a, const EvalImage& im, float thr, int lane, Write write) {
    const int G = im.G, ns = im.ns;
    const int passes = (G + 63) >> 6;                        // <= EV_MAX_GT / 64 = 16 bits of `matched`
    unsigned int matched = 0;                                // bit p: ground-truth box p * 64 + lane is taken
    for (int d0 = 0; d0 < ns; d0 += 64) {
        const int d = d0 + lane;
        const bool have = d < ns;
        const unsigned int lo = have ? ev_key_word(L, d, 0) : 0u;
        const int my_row = (int)(lo >> 8), my_cls = (int)(lo & 255u);
        const float* r = im.rows + (size_t)my_row * a.D;
        NBox me = make_box(0.f, 0.f, 0.f, 0.f);
        if (have) me = make_box(r[0], r[1], r[2], r[3]);
        int my_tp = 0, my_gt = -1;
        float my_iou = 0.f;
        const int nd = min(64, ns - d0);
        for (int j = 0; j < nd; ++j) {
            NBox o;
            o.y0 = __shfl(me.y0, j); o.x0 = __shfl(me.x0, j); o.y1 = __shfl(me.y1, j); o.x1 = __shfl(me.x1, j);
            o.area = __shfl(me.area, j);
            const int oc = __shfl(my_cls, j);
            float bi = -1.f;                                 // best of this lane's boxes: strictly larger wins, so the lower pass
            int bg = 0x7fffffff;
            for (int p = 0; p < passes; ++p) {
                const int g = (p << 6) + lane;
                if (g < G && L.label[g] == oc && !((matched >> p) & 1u)) {
                    NBox q; q.y0 = L.y0[g]; q.x0 = L.x0[g]; q.y1 = L.y1[g]; q.x1 = L.x1[g]; q.area = L.ar[g];
                    float v = iou_value(o, q);
                    if (!(v >= 0.f)) v = 0.f;                // non-finite coordinates: no overlap
                    if (v > bi) { bi = v; bg = g; }
                }
            }
#pragma unroll
            for (int sft = 1; sft < 64; sft <<= 1) {         // arg-max over the lanes: larger IoU, then lower index
                const float vi = __shfl_xor(bi, sft);
                const int vg = __shfl_xor(bg, sft);
                if (vi > bi || (vi == bi && vg < bg)) { bi = vi; bg = vg; }
            }
            const bool any = bg != 0x7fffffff;
            const bool tp = any && bi >= thr;
            if (tp && (bg & 63) == lane) matched |= 1u << (bg >> 6);
            if (lane == j) { my_tp = tp ? 1 : 0; my_gt = tp ? bg : -1; my_iou = any ? bi : 0.f; }
        }
        if (have) write(d, my_row, my_cls, r, my_tp, my_gt, my_iou);
    }
}

__global__ __launch_bounds__(64) void eval_match_kernel(const EvalArgs a) {
    __shared__ EvalLds L;
    const int b = blockIdx.x, lane = threadIdx.x;
    const EvalImage im = ev_stage_and_sort<true>(L, a, b, lane, 64);
    // 6 -- the record
    ev_greedy_pass(L, a, im, a.iou_thresh, lane, [&](int d, int row, int cls, const float* r, int tp, int gt, float iou) {
        const long long pos = im.base + d;
        if (pos < a.capacity) {
            int32_t* w = a.table + (size_t)pos * (EV_HEAD + a.n_unc);
            w[0] = a.img_base + b; w[1] = row; w[2] = cls;
            w[3] = __float_as_int(__fmul_rn(r[a.obj_idx], r[a.cls_start + cls]));
            w[4] = tp; w[5] = gt; w[6] = __float_as_int(iou);
#pragma unroll
            for (int u = 0; u < EV_MAX_UNC; ++u)
                if (u < a.n_unc) w[EV_HEAD + u] = __float_as_int(r[a.unc[u]]);
        } else {
            a.state[ST_OVERFLOW] = 1;                        // sticky: nothing clears it but byolo_eval_reset
        }
    });
}

// ---- the ladder: the matching at several IoU thresholds ---------------------------------------------------------------------
struct LadderArgs {
    EvalArgs e;                                                  // table is not written, state is read only
    int32_t* ladder;
    int32_t n_thr;
    float thr[LAD_MAX];
};

struct LadderLds {
    EvalLds L;
    float thr[LAD_MAX];
};

__global__ __launch_bounds__(64 * LAD_MAX) void eval_ladder_kernel(const LadderArgs la) {
    __shared__ LadderLds S;
    EvalLds& L = S.L;
    const EvalArgs& a = la.e;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nthreads = 64 * la.n_thr;
    if (tid < la.n_thr) S.thr[tid] = la.thr[tid];
    const EvalImage im = ev_stage_and_sort<false>(L, a, blockIdx.x, tid, nthreads);
    // the score half of a key has done its work: it collects the detection's true-positive bits
    for (int d = tid; d < im.ns; d += nthreads) ev_key_word(L, d, 1) = 0u;
    __syncthreads();

    // 6 -- this wave's threshold: its bit, and the box it matched
    const int rec_words = 1 + la.n_thr;
    ev_greedy_pass(L, a, im, S.thr[wave], lane, [&](int d, int, int, const float*, int tp, int gt, float) {
        const long long pos = im.base + d;
        if (tp) atomicOr(&ev_key_word(L, d, 1), 1u << wave);     // LDS
        if (pos < a.capacity) la.ladder[(size_t)pos * rec_words + 1 + wave] = gt;
    });
    __syncthreads();
    // word 0: the bits of every threshold
    for (int d = tid; d < im.ns; d += nthreads) {
        const long long pos = im.base + d;
        if (pos < a.capacity) la.ladder[(size_t)pos * rec_words] = (int32_t)ev_key_word(L, d, 1);
    }
}

// ---- the subsets: the matching per height range of the ground truth, with ignore regions ----------------------------------------
static constexpr int SUB_MAX = BYOLO_EVAL_SUBSETS_MAX;          // subsets = waves of the workgroup

struct SubsetArgs {
    EvalArgs e;                                                  // table is not written, state is read only
    int32_t* sub;                                                // 1 + n_sub words per record
    int32_t* counts;                                             // n_sub * C: the counted boxes per (subset, class)
    int32_t n_sub, other;
    float img_h, ignore_thresh, slack;
    float lo[SUB_MAX], hi[SUB_MAX];
};

struct SubsetLds {
    EvalLds L;
    float lo[SUB_MAX], hi[SUB_MAX];
};

// pixel height of a box made by make_box
__device__ __forceinline__ float ev_height(float y0, float y1, float img_h) { return __fmul_rn(__fsub_rn(y1, y0), img_h); }

// arg-max over the lanes: larger value, then lower index; every lane ends with the result
__device__ __forceinline__ void ev_argmax(float& bi, int& bg) {
#pragma unroll
    for (int sft = 1; sft < 64; sft <<= 1) {
        const float vi = __shfl_xor(bi, sft);
        const int vg = __shfl_xor(bg, sft);
        if (vi > bi || (vi == bi && vg < bg)) { bi = vi; bg = vg; }
    }
}

// 5' -- the pass of one wave for the subset [lo, hi): the walk of ev_greedy_pass with two searches per detection.  A box is
// COUNTED when its label is a class and its height is inside the range; a detection takes the counted, not yet matched box of
// its class with the largest IoU (state 1 iff that IoU >= thr); failing that it looks for the ignore region -- a box without a
// class, a box of its class that is not counted, with `other` a box of another class -- that covers most of the detection's own
// area (state 2 iff inter / det.area >= ignore_thresh; regions are never used up); failing that its own height decides between
// state 3 (outside [lo / slack, hi * slack)) and 0.  Every detection's lane hands write(d, state, box or region or -1).
// Adds the counted boxes to counts[0 .. C).
template <class Write>
__device__ __forceinline__ void ev_subset_pass(EvalLds& L, const SubsetArgs& sa, const EvalImage& im, float lo_s, float hi_s, int32_t* counts,
                                               int lane, Write write) {
    const EvalArgs& a = sa.e;
    const int G = im.G, ns = im.ns;
    const int passes = (G + 63) >> 6;                        // <= EV_MAX_GT / 64 = 16 bits of `matched` and `counted`
    const float dlo = __fdiv_rn(lo_s, sa.slack), dhi = __fmul_rn(hi_s, sa.slack);
    unsigned int counted = 0;                                // bit p: ground-truth box p * 64 + lane is counted in this subset
    for (int p = 0; p < passes; ++p) {
        const int g = (p << 6) + lane;
        if (g < G && L.label[g] >= 0) {
            const float h = ev_height(L.y0[g], L.y1[g], sa.img_h);
            if (h >= lo_s && h < hi_s) {                     // a NaN height fails the first comparison
                counted |= 1u << p;
                atomicAdd(&counts[L.label[g]], 1);
            }
        }
    }
    unsigned int matched = 0;                                // bit p: ground-truth box p * 64 + lane is taken
    for (int d0 = 0; d0 < ns; d0 += 64) {
        const int d = d0 + lane;
        const bool have = d < ns;
        const unsigned int kw = have ? ev_key_word(L, d, 0) : 0u;
        const int my_row = (int)(kw >> 8), my_cls = (int)(kw & 255u);
        const float* r = im.rows + (size_t)my_row * a.D;
        NBox me = make_box(0.f, 0.f, 0.f, 0.f);
        if (have) me = make_box(r[0], r[1], r[2], r[3]);
        int my_state = 0, my_ref = -1;
        const int nd = min(64, ns - d0);
        for (int j = 0; j < nd; ++j) {
            NBox o;
            o.y0 = __shfl(me.y0, j); o.x0 = __shfl(me.x0, j); o.y1 = __shfl(me.y1, j); o.x1 = __shfl(me.x1, j);
            o.area = __shfl(me.area, j);
            const int oc = __shfl(my_cls, j);
            float bi = -1.f, ri = -1.f;                      // best counted box / best region of this lane's boxes
            int bg = 0x7fffffff, rg = 0x7fffffff;
            for (int p = 0; p < passes; ++p) {
                const int g = (p << 6) + lane;
                if (g >= G) continue;
                const int lab = L.label[g];
                const bool cnt = (counted >> p) & 1u;
                const bool open = lab == oc && cnt && !((matched >> p) & 1u);
                const bool region = lab < 0 || (lab == oc ? !cnt : sa.other != 0);
                if (!open && !region) continue;
                NBox q; q.y0 = L.y0[g]; q.x0 = L.x0[g]; q.y1 = L.y1[g]; q.x1 = L.x1[g]; q.area = L.ar[g];
                if (open) {
                    float v = iou_value(o, q);
                    if (!(v >= 0.f)) v = 0.f;                // non-finite coordinates: no overlap
                    if (v > bi) { bi = v; bg = g; }
                } else {
                    float v = 0.f;
                    if (!(o.area <= 0.f || q.area <= 0.f)) {
                        const float iy0 = smax_(o.y0, q.y0), ix0 = smax_(o.x0, q.x0);
                        const float iy1 = smin_(o.y1, q.y1), ix1 = smin_(o.x1, q.x1);
                        const float inter = __fmul_rn(smax_(__fsub_rn(iy1, iy0), 0.f), smax_(__fsub_rn(ix1, ix0), 0.f));
                        v = __fdiv_rn(inter, o.area);
                    }
                    if (!(v >= 0.f && v <= FLT_MAX)) v = 0.f;
                    if (v > ri) { ri = v; rg = g; }
                }
            }
            // a search succeeds iff some lane's best reaches the threshold, and then the winner is among those lanes: the
            // arg-max runs only where its result is used.  The branches are uniform: the ballots are the wave's
            int state = 0, ref = -1;
            if (__ballot(bg != 0x7fffffff && bi >= a.iou_thresh)) {
                ev_argmax(bi, bg);
                state = 1; ref = bg;
                if ((bg & 63) == lane) matched |= 1u << (bg >> 6);
            } else {
                if (__ballot(rg != 0x7fffffff && ri >= sa.ignore_thresh)) {
                    ev_argmax(ri, rg);
                    state = 2; ref = rg;
                } else {
                    const float h = ev_height(o.y0, o.y1, sa.img_h);
                    if (h < dlo || h >= dhi) state = 3;      // a NaN height fails both: a false positive
                }
            }
            if (lane == j) { my_state = state; my_ref = ref; }
        }
        if (have) write(d, my_state, my_ref);
    }
}

__global__ __launch_bounds__(64 * SUB_MAX) void eval_subset_kernel(const SubsetArgs sa) {
    __shared__ SubsetLds S;
    EvalLds& L = S.L;
    const EvalArgs& a = sa.e;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nthreads = 64 * sa.n_sub;
    if (tid < sa.n_sub) { S.lo[tid] = sa.lo[tid]; S.hi[tid] = sa.hi[tid]; }
    const EvalImage im = ev_stage_and_sort<false>(L, a, blockIdx.x, tid, nthreads);
    // the score half of a key has done its work: it collects the detection's 2-bit states
    for (int d = tid; d < im.ns; d += nthreads) ev_key_word(L, d, 1) = 0u;
    __syncthreads();

    // 6 -- this wave's subset: its state, and the box or region behind it
    const int rec_words = 1 + sa.n_sub;
    ev_subset_pass(L, sa, im, S.lo[wave], S.hi[wave], sa.counts + (size_t)wave * a.C, lane, [&](int d, int state, int ref) {
        const long long pos = im.base + d;
        if (state) atomicOr(&ev_key_word(L, d, 1), (unsigned int)state << (2 * wave));     // LDS
        if (pos < a.capacity) sa.sub[(size_t)pos * rec_words + 1 + wave] = ref;
    });
    __syncthreads();
    // word 0: the states of every subset
    for (int d = tid; d < im.ns; d += nthreads) {
        const long long pos = im.base + d;
        if (pos < a.capacity) sa.sub[(size_t)pos * rec_words] = (int32_t)ev_key_word(L, d, 1);
    }
}

// ---- localisation residuals --------------------------------------------------------------------------------------------------
static constexpr int LOC_WORDS = BYOLO_EVAL_LOC_WORDS;
static constexpr int LOC_L = BYOLO_EVAL_LOC_MAX_LAYERS, LOC_P = BYOLO_EVAL_LOC_MAX_PRIORS;

struct LocArgs {
    const float* rows; const float* gt_boxes; const int32_t* table; const int32_t* state; int32_t* loc; int64_t capacity;
    int32_t B, cap, D, gmax, rec_words, parity, img_base, layer_col, prior_col, n_layers;
    int32_t lh[LOC_L], lw[LOC_L], n_priors[LOC_L];
    float pw[LOC_L][LOC_P], ph[LOC_L][LOC_P];
};

// an id column: finite, integral and inside [0, n)
__device__ __forceinline__ bool loc_id(float v, int n, int& id) {
    const bool ok = v >= 0.f && v < (float)n && floorf(v) == v;      // NaN and inf fail the comparisons
    id = ok ? (int)v : 0;
    return ok;
}

// centre coordinate: the cell and the detection's and the ground truth's offsets inside it (float64, one operation per line)
__device__ __forceinline__ void loc_centre(double lo, double hi, double glo, double ghi, int n, int& cell, double& p, double& q) {
    const double c = (lo + hi) * 0.5;
    const double s = c * (double)n;
    double f = floor(s);
    if (!(f >= 0.0)) f = 0.0;                                         // NaN lands in cell 0 and fails the validity test
    if (f > (double)(n - 1)) f = (double)(n - 1);
    cell = (int)f;
    p = s - f;
    const double g = (glo + ghi) * 0.5;
    q = g * (double)n - f;
}

__device__ __forceinline__ double loc_logit(double p) {
    const double m = 1.0 - p;
    const double r = p / m;
    return log(r);
}

__global__ __launch_bounds__(256) void eval_loc_kernel(const LocArgs a) {
    constexpr double EPS = 1e-7;
    const long long first = a.state[ST_TOTAL0 + a.parity];
    long long last = a.state[ST_TOTAL0 + (a.parity ^ 1)];
    if (last > a.capacity) last = a.capacity;
    const long long pos = first + (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (pos < 0 || pos >= last) return;
    const int32_t* w = a.table + (size_t)pos * a.rec_words;
    const int b = w[0] - a.img_base, row = w[1], tp = w[4], gt = w[5];
    float r[4] = {0.f, 0.f, 0.f, 0.f};
    int flags = 0, cell = 0;
    if (b >= 0 && b < a.B && row >= 0 && row < a.cap) {
        const float* d = a.rows + ((size_t)b * a.cap + row) * a.D;
        int layer, prior = 0;
        bool ids = loc_id(d[a.layer_col], a.n_layers, layer);
        if (ids) ids = loc_id(d[a.prior_col], a.n_priors[layer], prior);
        if (tp == 1) flags |= 16;
        if (ids) flags |= 32 | (layer << 8) | (prior << 16);
        if (ids && tp == 1 && gt >= 0 && gt < a.gmax) {
            const float* g = a.gt_boxes + ((size_t)b * a.gmax + gt) * 4;
            const int lh = a.lh[layer], lw = a.lw[layer];
            const double pw = (double)a.pw[layer][prior], ph = (double)a.ph[layer][prior];
            const double y0 = d[0], x0 = d[1], y1 = d[2], x1 = d[3];
            const double gy0 = g[0], gx0 = g[1], gy1 = g[2], gx1 = g[3];
            int ix, iy;
            double px, qx, py, qy;
            loc_centre(x0, x1, gx0, gx1, lw, ix, px, qx);
            loc_centre(y0, y1, gy0, gy1, lh, iy, py, qy);
            cell = iy * lw + ix;
            if (px >= EPS && px <= 1.0 - EPS && qx >= EPS && qx <= 1.0 - EPS) {
                r[0] = (float)(loc_logit(qx) - loc_logit(px));
                flags |= 1;
            }
            if (py >= EPS && py <= 1.0 - EPS && qy >= EPS && qy <= 1.0 - EPS) {
                r[1] = (float)(loc_logit(qy) - loc_logit(py));
                flags |= 2;
            }
            const double dw = (x1 - x0) / pw, gw = (gx1 - gx0) / pw;
            if (dw >= EPS && gw >= EPS) {
                r[2] = (float)(log(gw) - log(dw));
                flags |= 4;
            }
            const double dh = (y1 - y0) / ph, gh = (gy1 - gy0) / ph;
            if (dh >= EPS && gh >= EPS) {
                r[3] = (float)(log(gh) - log(dh));
                flags |= 8;
            }
        }
    }
    int32_t* o = a.loc + (size_t)pos * LOC_WORDS;
    o[0] = __float_as_int(r[0]); o[1] = __float_as_int(r[1]); o[2] = __float_as_int(r[2]); o[3] = __float_as_int(r[3]);
    o[4] = flags; o[5] = cell;
}

}  // namespace byk

// ---- C-ABI --------------------------------------------------------------------------------------------------------------
struct byolo_eval {
    byolo_eval_cfg cfg;
    int32_t* d_table = nullptr;
    int32_t* d_state = nullptr;
    int64_t capacity = 0;
    int32_t launches = 0;
    int64_t images = 0;
    byolo_eval_loc_cfg loc;                                     // valid while d_loc is set (byolo_eval_set_loc)
    int32_t* d_loc = nullptr;
    byolo_eval_ladder_cfg ladder;                               // valid while d_ladder is set (byolo_eval_set_ladder)
    int32_t* d_ladder = nullptr;
    byolo_eval_subsets_cfg subsets;                             // valid while d_subsets is set (byolo_eval_set_subsets)
    int32_t* d_subsets = nullptr;
    int32_t* d_subset_counts = nullptr;
    byk::PdqSide pdq;                                           // valid while pdq.d_images is set (byolo_eval_set_pdq)
    std::string err;
};

static thread_local std::string g_eval_err;

int32_t byk::efail(byolo_eval_t* ev, int32_t code, const char* fmt, ...) {     // eval_pdq.h: csrc/eval_pdq.hip reports through it too
    char buf[512];
    va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
    if (ev) ev->err = buf; else g_eval_err = buf;
    return code;
}
using byk::efail;
#define EVHIP(ev, call) do { hipError_t e_ = (call); if (e_ != hipSuccess) \
    return efail(ev, BYOLO_ERR_HIP, "%s failed: %s", #call, hipGetErrorString(e_)); } while (0)

static int state_words(int C) { return byk::ST_CLASS0 + C; }
static int record_words(const byolo_eval_cfg& c) { return byk::EV_HEAD + c.n_unc; }

extern "C" const char* byolo_eval_last_error(const byolo_eval_t* ev) { return ev ? ev->err.c_str() : g_eval_err.c_str(); }

extern "C" size_t byolo_eval_state_bytes(int32_t cls_cnt) {
    return cls_cnt < 1 ? 0 : sizeof(int32_t) * (size_t)state_words(cls_cnt);
}

extern "C" int32_t byolo_eval_create(const byolo_eval_cfg* cfg, void* d_table, int64_t capacity, void* d_state, byolo_eval_t** out) {
    if (!cfg || !out || !d_table || !d_state) return efail(nullptr, BYOLO_ERR_ARG, "byolo_eval_create: null argument");
    if (cfg->struct_bytes != (int32_t)sizeof(byolo_eval_cfg))
        return efail(nullptr, BYOLO_ERR_ARG, "byolo_eval_create: struct_bytes %d, this library's byolo_eval_cfg has %d", cfg->struct_bytes, (int)sizeof(byolo_eval_cfg));
    if (cfg->cls_cnt < 1 || cfg->cls_cnt > BYOLO_NMS_MAX_CLASSES) return efail(nullptr, BYOLO_ERR_ARG, "byolo_eval_create: cls_cnt outside 1 .. %d", BYOLO_NMS_MAX_CLASSES);
    if (cfg->row_len < 5 || cfg->obj_idx < 4 || cfg->obj_idx >= cfg->row_len || cfg->cls_start_idx < 4 ||
        (int64_t)cfg->cls_start_idx + cfg->cls_cnt > cfg->row_len)
        return efail(nullptr, BYOLO_ERR_ARG, "byolo_eval_create: score columns outside the row");
    if (cfg->n_unc < 0 || cfg->n_unc > BYOLO_EVAL_MAX_UNC) return efail(nullptr, BYOLO_ERR_ARG, "byolo_eval_create: n_unc outside 0 .. %d", BYOLO_EVAL_MAX_UNC);
    for (int u = 0; u < cfg->n_unc; ++u)
        if (cfg->unc_cols[u] < 0 || cfg->unc_cols[u] >= cfg->row_len) return efail(nullptr, BYOLO_ERR_ARG, "byolo_eval_create: uncertainty column %d outside the row", cfg->unc_cols[u]);
    if (!(cfg->iou_thresh >= 0.f && cfg->iou_thresh <= 1.f)) return efail(nullptr, BYOLO_ERR_ARG, "byolo_eval_create: iou_thresh outside [0, 1]");
    if (cfg->min_score != cfg->min_score) return efail(nullptr, BYOLO_ERR_ARG, "byolo_eval_create: min_score is NaN");
    if (capacity < 1 || capacity > 0x7fffffffll) return efail(nullptr, BYOLO_ERR_ARG, "byolo_eval_create: capacity outside 1 .. 2^31 - 1 records");
    if ((reinterpret_cast<uintptr_t>(d_table) | reinterpret_cast<uintptr_t>(d_state)) & 3) return efail(nullptr, BYOLO_ERR_ARG, "byolo_eval_create: d_table / d_state must be 4-byte aligned");
    byolo_eval_t* ev = new (std::nothrow) byolo_eval();
    if (!ev) return efail(nullptr, BYOLO_ERR_NOMEM, "byolo_eval_create: out of host memory");
    ev->cfg = *cfg;
    ev->d_table = static_cast<int32_t*>(d_table);
    ev->d_state = static_cast<int32_t*>(d_state);
    ev->capacity = capacity;
    *out = ev;
    return BYOLO_OK;
}

extern "C" int32_t byolo_eval_destroy(byolo_eval_t* ev) { delete ev; return BYOLO_OK; }

extern "C" int32_t byolo_eval_reset(byolo_eval_t* ev, void* stream) {
    if (!ev) return efail(nullptr, BYOLO_ERR_ARG, "byolo_eval_reset: null handle");
    EVHIP(ev, hipMemsetAsync(ev->d_state, 0, sizeof(int32_t) * (size_t)state_words(ev->cfg.cls_cnt), static_cast<hipStream_t>(stream)));
    if (ev->d_subsets)
        EVHIP(ev, hipMemsetAsync(ev->d_subset_counts, 0, sizeof(int32_t) * (size_t)ev->subsets.n_subsets * (size_t)ev->cfg.cls_cnt,
                                 static_cast<hipStream_t>(stream)));
    if (ev->pdq.d_images)
        EVHIP(ev, hipMemsetAsync(ev->pdq.d_state, 0, byolo_eval_pdq_state_bytes(), static_cast<hipStream_t>(stream)));
    ev->launches = 0;
    ev->images = 0;
    return BYOLO_OK;
}

extern "C" int32_t byolo_eval_add(byolo_eval_t* ev, const float* d_rows, int32_t B, int32_t cap, const int32_t* d_count, int64_t count_stride,
                                  const float* d_gt_boxes, const int32_t* d_gt_labels, const int32_t* d_gt_counts, int32_t gmax, void* stream) {
    if (!ev) return efail(nullptr, BYOLO_ERR_ARG, "byolo_eval_add: null handle");
    if (!d_rows || !d_count || !d_gt_boxes || !d_gt_labels || !d_gt_counts) return efail(ev, BYOLO_ERR_ARG, "byolo_eval_add: null argument");
    if (B < 1 || B > 65535) return efail(ev, BYOLO_ERR_ARG, "byolo_eval_add: B outside 1 .. 65535");
    if (cap < 1 || cap > byk::EV_MAX_DET) return efail(ev, BYOLO_ERR_ARG, "byolo_eval_add: cap outside 1 .. %d rows per image", byk::EV_MAX_DET);
    if (gmax < 1 || gmax > BYOLO_EVAL_MAX_GT) return efail(ev, BYOLO_ERR_ARG, "byolo_eval_add: gmax outside 1 .. %d boxes per image", BYOLO_EVAL_MAX_GT);
    if (count_stride < 1) return efail(ev, BYOLO_ERR_ARG, "byolo_eval_add: count_stride below 1");
    if (ev->images + B > 0x7fffffffll) return efail(ev, BYOLO_ERR_ARG, "byolo_eval_add: more than 2^31 - 1 images");
    if (ev->pdq.d_images && byk::pdq_workspace_bytes(B, cap, gmax) > ev->pdq.ws_bytes)
        return efail(ev, BYOLO_ERR_NOMEM, "byolo_eval_add: the PDQ workspace holds %zu bytes, this batch needs byolo_eval_pdq_workspace_bytes(%d, %d, %d) = %zu",
                     ev->pdq.ws_bytes, B, cap, gmax, byk::pdq_workspace_bytes(B, cap, gmax));
    byk::EvalArgs a;
    a.rows = d_rows; a.count = d_count; a.count_stride = count_stride;
    a.gt_boxes = d_gt_boxes; a.gt_labels = d_gt_labels; a.gt_counts = d_gt_counts;
    a.table = ev->d_table; a.state = ev->d_state; a.capacity = ev->capacity;
    a.B = B; a.cap = cap; a.D = ev->cfg.row_len; a.obj_idx = ev->cfg.obj_idx; a.cls_start = ev->cfg.cls_start_idx; a.C = ev->cfg.cls_cnt;
    a.gmax = gmax; a.n_unc = ev->cfg.n_unc; a.parity = ev->launches & 1; a.img_base = (int32_t)ev->images;
    a.iou_thresh = ev->cfg.iou_thresh; a.min_score = ev->cfg.min_score;
    for (int u = 0; u < BYOLO_EVAL_MAX_UNC; ++u) a.unc[u] = u < ev->cfg.n_unc ? ev->cfg.unc_cols[u] : 0;
    hipLaunchKernelGGL(byk::eval_match_kernel, dim3(B), dim3(64), 0, static_cast<hipStream_t>(stream), a);
    EVHIP(ev, hipGetLastError());
    if (ev->d_loc) {                                            // the launch's records are final once the match kernel has ended
        byk::LocArgs l;
        l.rows = d_rows; l.gt_boxes = d_gt_boxes; l.table = ev->d_table; l.state = ev->d_state; l.loc = ev->d_loc; l.capacity = ev->capacity;
        l.B = B; l.cap = cap; l.D = ev->cfg.row_len; l.gmax = gmax; l.rec_words = record_words(ev->cfg); l.parity = a.parity; l.img_base = a.img_base;
        l.layer_col = ev->loc.layer_col; l.prior_col = ev->loc.prior_col; l.n_layers = ev->loc.n_layers;
        for (int k = 0; k < byk::LOC_L; ++k) {
            l.lh[k] = ev->loc.lh[k]; l.lw[k] = ev->loc.lw[k]; l.n_priors[k] = ev->loc.n_priors[k];
            for (int q = 0; q < byk::LOC_P; ++q) { l.pw[k][q] = ev->loc.prior_w[k][q]; l.ph[k][q] = ev->loc.prior_h[k][q]; }
        }
        const int64_t threads = (int64_t)B * cap;               // <= 65535 * 4096
        hipLaunchKernelGGL(byk::eval_loc_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), l);
        EVHIP(ev, hipGetLastError());
    }
    if (ev->d_ladder) {                                         // reads the offset word the match kernel leaves alone
        byk::LadderArgs la;
        la.e = a;
        la.e.table = nullptr;
        la.ladder = ev->d_ladder;
        la.n_thr = ev->ladder.n_thr;
        for (int k = 0; k < byk::LAD_MAX; ++k) la.thr[k] = k < la.n_thr ? ev->ladder.thresholds[k] : 0.f;
        hipLaunchKernelGGL(byk::eval_ladder_kernel, dim3(B), dim3(64 * la.n_thr), 0, static_cast<hipStream_t>(stream), la);
        EVHIP(ev, hipGetLastError());
    }
    if (ev->d_subsets) {                                        // likewise; the main table and the state are only read
        byk::SubsetArgs sa;
        sa.e = a;
        sa.e.table = nullptr;
        sa.sub = ev->d_subsets;
        sa.counts = ev->d_subset_counts;
        sa.n_sub = ev->subsets.n_subsets;
        sa.other = ev->subsets.ignore_other_classes ? 1 : 0;
        sa.img_h = ev->subsets.img_h; sa.ignore_thresh = ev->subsets.ignore_thresh; sa.slack = ev->subsets.height_slack;
        for (int k = 0; k < byk::SUB_MAX; ++k) {
            sa.lo[k] = k < sa.n_sub ? ev->subsets.lo[k] : 0.f;
            sa.hi[k] = k < sa.n_sub ? ev->subsets.hi[k] : 0.f;
        }
        hipLaunchKernelGGL(byk::eval_subset_kernel, dim3(B), dim3(64 * sa.n_sub), 0, static_cast<hipStream_t>(stream), sa);
        EVHIP(ev, hipGetLastError());
    }
    if (ev->pdq.d_images) {                                     // csrc/eval_pdq.hip: reads the rows and the ground truth, none of the tables above
        byk::PdqBatch pb;
        pb.rows = d_rows; pb.count = d_count; pb.count_stride = count_stride;
        pb.gt_boxes = d_gt_boxes; pb.gt_labels = d_gt_labels; pb.gt_counts = d_gt_counts;
        pb.B = B; pb.cap = cap; pb.D = ev->cfg.row_len; pb.obj_idx = ev->cfg.obj_idx; pb.cls_start = ev->cfg.cls_start_idx; pb.C = ev->cfg.cls_cnt;
        pb.gmax = gmax; pb.img_base = a.img_base;
        EVHIP(ev, byk::pdq_launch(ev->pdq, pb, static_cast<hipStream_t>(stream)));
        ev->pdq.last_B = B; ev->pdq.last_cap = cap; ev->pdq.last_gmax = gmax;
    }
    ev->launches += 1;
    ev->images += B;
    return BYOLO_OK;
}

extern "C" int32_t byolo_eval_finish(byolo_eval_t* ev, byolo_eval_summary* out, int64_t* h_class_gt, int32_t n_classes, void* stream) {
    if (!ev) return efail(nullptr, BYOLO_ERR_ARG, "byolo_eval_finish: null handle");
    if (!out || !h_class_gt) return efail(ev, BYOLO_ERR_ARG, "byolo_eval_finish: null argument");
    if (out->struct_bytes != (int32_t)sizeof(byolo_eval_summary))
        return efail(ev, BYOLO_ERR_ARG, "byolo_eval_finish: struct_bytes %d, this library's byolo_eval_summary has %d", out->struct_bytes, (int)sizeof(byolo_eval_summary));
    if (n_classes != ev->cfg.cls_cnt) return efail(ev, BYOLO_ERR_ARG, "byolo_eval_finish: h_class_gt has %d entries, the evaluator %d classes", n_classes, ev->cfg.cls_cnt);
    int32_t st[byk::ST_CLASS0 + BYOLO_NMS_MAX_CLASSES];
    hipStream_t s = static_cast<hipStream_t>(stream);
    EVHIP(ev, hipMemcpyAsync(st, ev->d_state, sizeof(int32_t) * (size_t)state_words(n_classes), hipMemcpyDeviceToHost, s));
    EVHIP(ev, hipStreamSynchronize(s));
    const int64_t seen = st[byk::ST_TOTAL0 + (ev->launches & 1)];
    out->n_seen = seen;
    out->n_records = seen < ev->capacity ? seen : ev->capacity;
    out->n_images = st[byk::ST_IMAGES];
    out->overflow = st[byk::ST_OVERFLOW];
    out->record_words = record_words(ev->cfg);
    for (int c = 0; c < n_classes; ++c) h_class_gt[c] = st[byk::ST_CLASS0 + c];
    if (out->overflow || seen > ev->capacity)
        return efail(ev, BYOLO_ERR_NOMEM, "byolo_eval_finish: %lld detections, the record table holds %lld: the rest were dropped",
                     (long long)seen, (long long)ev->capacity);
    return BYOLO_OK;
}

// byolo_eval_records / _loc_records / _ladder_records / _subsets_records (fn): n_records records of `words` words from `first` of d_table on
static int32_t fetch_records(byolo_eval_t* ev, const char* fn, const int32_t* d_table, size_t words, int64_t first, int64_t n_records,
                             int32_t* h_dst, void* stream) {
    if (first < 0 || n_records < 0 || first + n_records > ev->capacity) return efail(ev, BYOLO_ERR_ARG, "%s: records outside the table", fn);
    if (n_records == 0) return BYOLO_OK;
    if (!h_dst) return efail(ev, BYOLO_ERR_ARG, "%s: null argument", fn);
    hipStream_t s = static_cast<hipStream_t>(stream);
    EVHIP(ev, hipMemcpyAsync(h_dst, d_table + (size_t)first * words, sizeof(int32_t) * words * (size_t)n_records, hipMemcpyDeviceToHost, s));
    EVHIP(ev, hipStreamSynchronize(s));
    return BYOLO_OK;
}

extern "C" int32_t byolo_eval_records(byolo_eval_t* ev, int32_t* h_dst, int64_t first, int64_t n_records, void* stream) {
    if (!ev) return efail(nullptr, BYOLO_ERR_ARG, "byolo_eval_records: null handle");
    return fetch_records(ev, "byolo_eval_records", ev->d_table, (size_t)record_words(ev->cfg), first, n_records, h_dst, stream);
}

// byolo_eval_set_loc / _set_ladder / _set_subsets (fn): everything around the checks of the cfg's own fields (`fields`: BYOLO_OK, or it has
// failed).  A NULL table switches the side table off
template <class Cfg, class Fields>
static int32_t set_side_table(byolo_eval_t* ev, const char* fn, const Cfg* cfg, const char* cfg_name, void* d_table, const char* table_name,
                              Cfg byolo_eval::*keep, int32_t* byolo_eval::*slot, Fields fields) {
    if (!ev) return efail(nullptr, BYOLO_ERR_ARG, "%s: null handle", fn);
    if (ev->launches) return efail(ev, BYOLO_ERR_STATE, "%s: records were added since the last byolo_eval_reset", fn);
    if (!d_table) { ev->*slot = nullptr; return BYOLO_OK; }
    if (!cfg) return efail(ev, BYOLO_ERR_ARG, "%s: null cfg", fn);
    if (cfg->struct_bytes != (int32_t)sizeof(Cfg))
        return efail(ev, BYOLO_ERR_ARG, "%s: struct_bytes %d, this library's %s has %d", fn, cfg->struct_bytes, cfg_name, (int)sizeof(Cfg));
    if (const int32_t rc = fields()) return rc;
    if (reinterpret_cast<uintptr_t>(d_table) & 3) return efail(ev, BYOLO_ERR_ARG, "%s: %s must be 4-byte aligned", fn, table_name);
    ev->*keep = *cfg;
    ev->*slot = static_cast<int32_t*>(d_table);
    return BYOLO_OK;
}

// ---- localisation residuals ------------------------------------------------------------------------------------------------
extern "C" size_t byolo_eval_loc_bytes(int64_t capacity) {
    return capacity < 1 || capacity > 0x7fffffffll ? 0 : sizeof(int32_t) * (size_t)byk::LOC_WORDS * (size_t)capacity;
}

extern "C" int32_t byolo_eval_set_loc(byolo_eval_t* ev, const byolo_eval_loc_cfg* cfg, void* d_loc_table) {
    return set_side_table(ev, "byolo_eval_set_loc", cfg, "byolo_eval_loc_cfg", d_loc_table, "d_loc_table", &byolo_eval::loc, &byolo_eval::d_loc, [&]() -> int32_t {
        if (cfg->layer_col < 0 || cfg->layer_col >= ev->cfg.row_len) return efail(ev, BYOLO_ERR_ARG, "byolo_eval_set_loc: layer_col %d outside the row", cfg->layer_col);
        if (cfg->prior_col < 0 || cfg->prior_col >= ev->cfg.row_len) return efail(ev, BYOLO_ERR_ARG, "byolo_eval_set_loc: prior_col %d outside the row", cfg->prior_col);
        if (cfg->n_layers < 1 || cfg->n_layers > BYOLO_EVAL_LOC_MAX_LAYERS) return efail(ev, BYOLO_ERR_ARG, "byolo_eval_set_loc: n_layers outside 1 .. %d", BYOLO_EVAL_LOC_MAX_LAYERS);
        for (int l = 0; l < cfg->n_layers; ++l) {
            if (cfg->n_priors[l] < 1 || cfg->n_priors[l] > BYOLO_EVAL_LOC_MAX_PRIORS)
                return efail(ev, BYOLO_ERR_ARG, "byolo_eval_set_loc: n_priors of layer %d outside 1 .. %d", l, BYOLO_EVAL_LOC_MAX_PRIORS);
            if (cfg->lh[l] < 1 || cfg->lw[l] < 1) return efail(ev, BYOLO_ERR_ARG, "byolo_eval_set_loc: grid of layer %d below 1 x 1", l);
            for (int p = 0; p < cfg->n_priors[l]; ++p) {
                const float w = cfg->prior_w[l][p], h = cfg->prior_h[l][p];
                if (!(w > 0.f && w <= 3.402823466e38f && h > 0.f && h <= 3.402823466e38f))
                    return efail(ev, BYOLO_ERR_ARG, "byolo_eval_set_loc: prior %d of layer %d is not finite and > 0", p, l);
            }
        }
        return BYOLO_OK;
    });
}

extern "C" int32_t byolo_eval_loc_records(byolo_eval_t* ev, int32_t* h_dst, int64_t first, int64_t n_records, void* stream) {
    if (!ev) return efail(nullptr, BYOLO_ERR_ARG, "byolo_eval_loc_records: null handle");
    if (!ev->d_loc) return efail(ev, BYOLO_ERR_STATE, "byolo_eval_loc_records: no loc table is set (byolo_eval_set_loc)");
    return fetch_records(ev, "byolo_eval_loc_records", ev->d_loc, byk::LOC_WORDS, first, n_records, h_dst, stream);
}

// ---- the ladder --------------------------------------------------------------------------------------------------------------
extern "C" size_t byolo_eval_ladder_bytes(int64_t capacity, int32_t n_thr) {
    if (capacity < 1 || capacity > 0x7fffffffll || n_thr < 1 || n_thr > BYOLO_EVAL_LADDER_MAX) return 0;
    return sizeof(int32_t) * (size_t)(1 + n_thr) * (size_t)capacity;
}

extern "C" int32_t byolo_eval_set_ladder(byolo_eval_t* ev, const byolo_eval_ladder_cfg* cfg, void* d_ladder_table) {
    return set_side_table(ev, "byolo_eval_set_ladder", cfg, "byolo_eval_ladder_cfg", d_ladder_table, "d_ladder_table", &byolo_eval::ladder, &byolo_eval::d_ladder, [&]() -> int32_t {
        if (cfg->n_thr < 1 || cfg->n_thr > BYOLO_EVAL_LADDER_MAX) return efail(ev, BYOLO_ERR_ARG, "byolo_eval_set_ladder: n_thr outside 1 .. %d", BYOLO_EVAL_LADDER_MAX);
        for (int k = 0; k < cfg->n_thr; ++k)
            if (!(cfg->thresholds[k] >= 0.f && cfg->thresholds[k] <= 1.f))
                return efail(ev, BYOLO_ERR_ARG, "byolo_eval_set_ladder: threshold %d is NaN or outside [0, 1]", k);
        return BYOLO_OK;
    });
}

extern "C" int32_t byolo_eval_ladder_records(byolo_eval_t* ev, int32_t* h_dst, int64_t first, int64_t n_records, void* stream) {
    if (!ev) return efail(nullptr, BYOLO_ERR_ARG, "byolo_eval_ladder_records: null handle");
    if (!ev->d_ladder) return efail(ev, BYOLO_ERR_STATE, "byolo_eval_ladder_records: no ladder table is set (byolo_eval_set_ladder)");
    return fetch_records(ev, "byolo_eval_ladder_records", ev->d_ladder, (size_t)(1 + ev->ladder.n_thr), first, n_records, h_dst, stream);
}

// ---- the subsets -------------------------------------------------------------------------------------------------------------
extern "C" size_t byolo_eval_subsets_bytes(int64_t capacity, int32_t n_subsets) {
    if (capacity < 1 || capacity > 0x7fffffffll || n_subsets < 1 || n_subsets > BYOLO_EVAL_SUBSETS_MAX) return 0;
    return sizeof(int32_t) * (size_t)(1 + n_subsets) * (size_t)capacity;
}

extern "C" size_t byolo_eval_subsets_state_bytes(int32_t n_subsets, int32_t cls_cnt) {
    if (n_subsets < 1 || n_subsets > BYOLO_EVAL_SUBSETS_MAX || cls_cnt < 1 || cls_cnt > BYOLO_NMS_MAX_CLASSES) return 0;
    return sizeof(int32_t) * (size_t)n_subsets * (size_t)cls_cnt;
}

extern "C" int32_t byolo_eval_set_subsets(byolo_eval_t* ev, const byolo_eval_subsets_cfg* cfg, void* d_subsets_table, void* d_subsets_counts) {
    const char* fn = "byolo_eval_set_subsets";
    return set_side_table(ev, fn, cfg, "byolo_eval_subsets_cfg", d_subsets_table, "d_subsets_table", &byolo_eval::subsets, &byolo_eval::d_subsets, [&]() -> int32_t {
        if (cfg->n_subsets < 1 || cfg->n_subsets > BYOLO_EVAL_SUBSETS_MAX) return efail(ev, BYOLO_ERR_ARG, "%s: n_subsets outside 1 .. %d", fn, BYOLO_EVAL_SUBSETS_MAX);
        for (int k = 0; k < cfg->n_subsets; ++k)
            if (!(cfg->lo[k] >= 0.f && cfg->lo[k] < cfg->hi[k]))                 // NaN fails both
                return efail(ev, BYOLO_ERR_ARG, "%s: height range %d is NaN, negative or inverted", fn, k);
        if (!(cfg->img_h > 0.f && cfg->img_h <= 3.402823466e38f)) return efail(ev, BYOLO_ERR_ARG, "%s: img_h is not finite and > 0", fn);
        if (!(cfg->ignore_thresh >= 0.f && cfg->ignore_thresh <= 1.f)) return efail(ev, BYOLO_ERR_ARG, "%s: ignore_thresh is NaN or outside [0, 1]", fn);
        if (!(cfg->height_slack >= 1.f && cfg->height_slack <= 3.402823466e38f)) return efail(ev, BYOLO_ERR_ARG, "%s: height_slack is not finite and >= 1", fn);
        if (!d_subsets_counts) return efail(ev, BYOLO_ERR_ARG, "%s: null d_subsets_counts", fn);
        if (reinterpret_cast<uintptr_t>(d_subsets_counts) & 3) return efail(ev, BYOLO_ERR_ARG, "%s: d_subsets_counts must be 4-byte aligned", fn);
        if (reinterpret_cast<uintptr_t>(d_subsets_table) & 3) return efail(ev, BYOLO_ERR_ARG, "%s: d_subsets_table must be 4-byte aligned", fn);
        ev->d_subset_counts = static_cast<int32_t*>(d_subsets_counts);       // the last check: nothing fails behind it
        return BYOLO_OK;
    });
}

extern "C" int32_t byolo_eval_subsets_records(byolo_eval_t* ev, int32_t* h_dst, int64_t first, int64_t n_records, void* stream) {
    if (!ev) return efail(nullptr, BYOLO_ERR_ARG, "byolo_eval_subsets_records: null handle");
    if (!ev->d_subsets) return efail(ev, BYOLO_ERR_STATE, "byolo_eval_subsets_records: no subsets table is set (byolo_eval_set_subsets)");
    return fetch_records(ev, "byolo_eval_subsets_records", ev->d_subsets, (size_t)(1 + ev->subsets.n_subsets), first, n_records, h_dst, stream);
}

extern "C" int32_t byolo_eval_subsets_counts(byolo_eval_t* ev, int64_t* h_counts, int32_t n_counts, void* stream) {
    if (!ev) return efail(nullptr, BYOLO_ERR_ARG, "byolo_eval_subsets_counts: null handle");
    if (!ev->d_subsets) return efail(ev, BYOLO_ERR_STATE, "byolo_eval_subsets_counts: no subsets table is set (byolo_eval_set_subsets)");
    const int n = ev->subsets.n_subsets * ev->cfg.cls_cnt;
    if (!h_counts || n_counts != n) return efail(ev, BYOLO_ERR_ARG, "byolo_eval_subsets_counts: h_counts has %d entries, the evaluator %d subsets x %d classes", n_counts, ev->subsets.n_subsets, ev->cfg.cls_cnt);
    int32_t st[BYOLO_EVAL_SUBSETS_MAX * BYOLO_NMS_MAX_CLASSES];
    hipStream_t s = static_cast<hipStream_t>(stream);
    EVHIP(ev, hipMemcpyAsync(st, ev->d_subset_counts, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, s));
    EVHIP(ev, hipStreamSynchronize(s));
    for (int k = 0; k < n; ++k) h_counts[k] = st[k];
    return BYOLO_OK;
}

// ---- probabilistic detection quality (csrc/eval_pdq.hip) ---------------------------------------------------------------------
extern "C" int32_t byolo_eval_set_pdq(byolo_eval_t* ev, const byolo_eval_pdq_cfg* cfg, const byolo_eval_loc_cfg* geom, void* d_image_table,
                                      int64_t image_capacity, void* d_pair_table, int64_t pair_capacity, void* d_state, void* d_workspace,
                                      size_t workspace_bytes) {
    const char* fn = "byolo_eval_set_pdq";
    if (!ev) return efail(nullptr, BYOLO_ERR_ARG, "%s: null handle", fn);
    if (ev->launches) return efail(ev, BYOLO_ERR_STATE, "%s: records were added since the last byolo_eval_reset", fn);
    if (!d_image_table) { ev->pdq.d_images = nullptr; return BYOLO_OK; }
    if (!cfg) return efail(ev, BYOLO_ERR_ARG, "%s: null cfg", fn);
    if (cfg->struct_bytes != (int32_t)sizeof(byolo_eval_pdq_cfg))
        return efail(ev, BYOLO_ERR_ARG, "%s: struct_bytes %d, this library's byolo_eval_pdq_cfg has %d", fn, cfg->struct_bytes, (int)sizeof(byolo_eval_pdq_cfg));
    if (const char* why = byk::pdq_check(cfg, geom, ev->cfg.row_len)) return efail(ev, BYOLO_ERR_ARG, "%s: %s", fn, why);
    if (image_capacity < 1 || image_capacity > 0x7fffffffll || pair_capacity < 1 || pair_capacity > 0x7fffffffll)
        return efail(ev, BYOLO_ERR_ARG, "%s: a capacity outside 1 .. 2^31 - 1 records", fn);
    if (!d_pair_table || !d_state || !d_workspace) return efail(ev, BYOLO_ERR_ARG, "%s: null d_pair_table / d_state / d_workspace", fn);
    if ((reinterpret_cast<uintptr_t>(d_image_table) | reinterpret_cast<uintptr_t>(d_pair_table) | reinterpret_cast<uintptr_t>(d_state) |
         reinterpret_cast<uintptr_t>(d_workspace)) & 7)
        return efail(ev, BYOLO_ERR_ARG, "%s: the tables, d_state and d_workspace must be 8-byte aligned", fn);
    EVHIP(ev, byk::pdq_prepare(*cfg));                          // the last thing that can fail, and before any batch is launched
    ev->pdq.cfg = *cfg;
    if (cfg->var != BYOLO_VOTE_NONE) ev->pdq.geom = *geom;
    ev->pdq.d_pairs = d_pair_table; ev->pdq.d_state = d_state; ev->pdq.d_ws = d_workspace;
    ev->pdq.image_capacity = image_capacity; ev->pdq.pair_capacity = pair_capacity; ev->pdq.ws_bytes = workspace_bytes;
    ev->pdq.d_images = d_image_table;
    ev->pdq.last_B = 0;
    return BYOLO_OK;
}

// The workspace carries nothing from one byolo_eval_add to the next, so it alone may be replaced at any time: the launches already on
// the stream keep the pointer they were given, which the caller keeps alive in stream order
extern "C" int32_t byolo_eval_set_pdq_workspace(byolo_eval_t* ev, void* d_workspace, size_t workspace_bytes) {
    const char* fn = "byolo_eval_set_pdq_workspace";
    if (!ev) return efail(nullptr, BYOLO_ERR_ARG, "%s: null handle", fn);
    if (!ev->pdq.d_images) return efail(ev, BYOLO_ERR_STATE, "%s: no PDQ tables are set (byolo_eval_set_pdq)", fn);
    if (!d_workspace) return efail(ev, BYOLO_ERR_ARG, "%s: null d_workspace", fn);
    if (reinterpret_cast<uintptr_t>(d_workspace) & 7) return efail(ev, BYOLO_ERR_ARG, "%s: d_workspace must be 8-byte aligned", fn);
    ev->pdq.d_ws = d_workspace;
    ev->pdq.ws_bytes = workspace_bytes;
    ev->pdq.last_B = 0;                                         // byolo_eval_pdq_matrix: the new workspace holds no batch yet
    return BYOLO_OK;
}

// byolo_eval_pdq_images / _pairs (fn): the count so far, then n_records records from `first` of d_table
static int32_t fetch_pdq(byolo_eval_t* ev, const char* fn, bool pairs, void* h_dst, int64_t first, int64_t n_records, int64_t* n_total, void* stream) {
    if (!ev) return efail(nullptr, BYOLO_ERR_ARG, "%s: null handle", fn);
    if (!ev->pdq.d_images) return efail(ev, BYOLO_ERR_STATE, "%s: no PDQ tables are set (byolo_eval_set_pdq)", fn);
    const int64_t capacity = pairs ? ev->pdq.pair_capacity : ev->pdq.image_capacity;
    if (first < 0 || n_records < 0 || first + n_records > capacity) return efail(ev, BYOLO_ERR_ARG, "%s: records outside the table", fn);
    if (n_records && !h_dst) return efail(ev, BYOLO_ERR_ARG, "%s: null argument", fn);
    hipStream_t s = static_cast<hipStream_t>(stream);
    int32_t st[byk::PDQ_ST_WORDS];
    EVHIP(ev, hipMemcpyAsync(st, ev->pdq.d_state, sizeof st, hipMemcpyDeviceToHost, s));
    if (n_records)
        EVHIP(ev, hipMemcpyAsync(h_dst, static_cast<const char*>(pairs ? ev->pdq.d_pairs : ev->pdq.d_images) + (size_t)first * BYOLO_PDQ_RECORD_BYTES,
                                 (size_t)n_records * BYOLO_PDQ_RECORD_BYTES, hipMemcpyDeviceToHost, s));
    EVHIP(ev, hipStreamSynchronize(s));
    unsigned long long cursor;
    memcpy(&cursor, st + byk::PDQ_ST_CURSOR, sizeof cursor);
    if (n_total) *n_total = pairs ? (int64_t)cursor : ev->images;
    const int flags = st[byk::PDQ_ST_FLAGS];
    if (flags)
        return efail(ev, BYOLO_ERR_NOMEM, "%s: %s%s%s", fn, flags & byk::PDQ_FLAG_DET ? "an image had more than 1024 detections at min_score; " : "",
                     flags & byk::PDQ_FLAG_IMAGES ? "more images than the image table holds; " : "",
                     flags & byk::PDQ_FLAG_PAIRS ? "more true positives than the pair table holds" : "");
    return BYOLO_OK;
}

extern "C" int32_t byolo_eval_pdq_images(byolo_eval_t* ev, void* h_dst, int64_t first, int64_t n_records, int64_t* n_total, void* stream) {
    return fetch_pdq(ev, "byolo_eval_pdq_images", false, h_dst, first, n_records, n_total, stream);
}

extern "C" int32_t byolo_eval_pdq_pairs(byolo_eval_t* ev, void* h_dst, int64_t first, int64_t n_records, int64_t* n_total, void* stream) {
    return fetch_pdq(ev, "byolo_eval_pdq_pairs", true, h_dst, first, n_records, n_total, stream);
}

extern "C" int32_t byolo_eval_pdq_matrix(byolo_eval_t* ev, int32_t image, int32_t* h_counts, int32_t* h_rows, int32_t* h_gts, double* h_planes, void* stream) {
    const char* fn = "byolo_eval_pdq_matrix";
    if (!ev) return efail(nullptr, BYOLO_ERR_ARG, "%s: null handle", fn);
    if (!ev->pdq.d_images || !ev->pdq.last_B) return efail(ev, BYOLO_ERR_STATE, "%s: no byolo_eval_add has run behind byolo_eval_set_pdq", fn);
    if (!h_counts || !h_rows || !h_gts || !h_planes) return efail(ev, BYOLO_ERR_ARG, "%s: null argument", fn);
    if (image < 0 || image >= ev->pdq.last_B) return efail(ev, BYOLO_ERR_ARG, "%s: image %d outside the last batch of %d", fn, image, ev->pdq.last_B);
    EVHIP(ev, byk::pdq_fetch_matrix(ev->pdq, ev->pdq.last_cap, ev->pdq.last_gmax, image, h_counts, h_rows, h_gts, h_planes, static_cast<hipStream_t>(stream)));
    return BYOLO_OK;
}
