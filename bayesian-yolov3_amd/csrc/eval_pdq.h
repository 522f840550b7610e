// eval_pdq.h -- what eval_kernels.hip (the evaluator's handle and C-ABI) and eval_pdq.hip (the PDQ kernels) share.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/byolo.h"

namespace byk {

// eval_kernels.hip: the message goes to the handle, or to the thread's slot without one
int32_t efail(byolo_eval_t* ev, int32_t code, const char* fmt, ...);

// the PDQ part of an evaluator: valid while d_images is set (byolo_eval_set_pdq)
struct PdqSide {
    byolo_eval_pdq_cfg cfg;
    byolo_eval_loc_cfg geom;                                 // read unless cfg.var == BYOLO_VOTE_NONE
    void* d_images = nullptr;
    void* d_pairs = nullptr;
    void* d_state = nullptr;
    void* d_ws = nullptr;                                    // scratch of ONE byolo_eval_add: may be replaced between two
    int64_t image_capacity = 0, pair_capacity = 0;
    size_t ws_bytes = 0;
    int32_t last_B = 0, last_cap = 0, last_gmax = 0;         // the last byolo_eval_add: what the workspace holds now
};

// one byolo_eval_add
struct PdqBatch {
    const float* rows; const int32_t* count; int64_t count_stride;
    const float* gt_boxes; const int32_t* gt_labels; const int32_t* gt_counts;
    int32_t B, cap, D, obj_idx, cls_start, C, gmax, img_base;
};

enum { PDQ_ST_CURSOR = 0 /* two words: uint64 */, PDQ_ST_FLAGS = 2, PDQ_ST_WORDS = 4 };
enum { PDQ_FLAG_DET = 1, PDQ_FLAG_IMAGES = 2, PDQ_FLAG_PAIRS = 4 };

size_t pdq_workspace_bytes(int B, int cap, int gmax);
// nullptr, or what is wrong with the settings (a printf format without arguments)
const char* pdq_check(const byolo_eval_pdq_cfg* cfg, const byolo_eval_loc_cfg* geom, int row_len);
// once per byolo_eval_set_pdq: raises the pair kernel's dynamic LDS limit where the frame needs it
hipError_t pdq_prepare(const byolo_eval_pdq_cfg& cfg);
// one image's slice of the workspace of a (B, cap, gmax) batch, copied out; waits for the stream
hipError_t pdq_fetch_matrix(const PdqSide& s, int cap, int gmax, int image, int32_t* h_counts, int32_t* h_rows, int32_t* h_gts, double* h_planes,
                            hipStream_t st);
hipError_t pdq_launch(const PdqSide& s, const PdqBatch& b, hipStream_t st);

}  // namespace byk
