/* byolo.h -- C-ABI of libbyolo.so: the MI355X-native (gfx950) Bayesian-YOLOv3 inference path.
 *
 * The reference (flkraus/bayesian-yolov3) has no FFI / plugin / operator interface: its hot path
 * sits behind Python function-level interfaces on top of the TensorFlow-1.x graph API.  This
 * header is therefore the boundary a maintainer would bind if the path were native: one entry
 * point per reference interface, each citing the reference symbol (file:line, relative to the
 * reference tree) it replaces.  INTEGRATION.md shows the ctypes binding.
 *
 * Conventions
 *   - every function returns int32 status: 0 = BYOLO_OK, negative = error; a message is
 *     available from byolo_last_error(handle) (handle-less failures: byolo_last_error(NULL));
 *   - no C++ exception crosses the ABI; no torch / HIP C++ types in signatures; `stream` is a
 *     hipStream_t passed as void* (NULL = the default stream);
 *   - all `d_*` pointers are CALLER-OWNED DEVICE memory (e.g. PyTorch-ROCm tensors); the library
 *     never frees them and never retains them past the call;  `h_*` pointers are host memory;
 *   - the library owns only the packed weights it uploads in byolo_finalize();
 *   - a handle is bound to one device and is not thread-safe: one handle per device/thread;
 *   - all tensors are float32, activations NHWC, convolution kernels HWIO
 *     (lib_yolo/layers.py:550, tf.layers.conv2d defaults), images in [0,1)
 *     (lib_yolo/dataset_utils.py:6-11).
 */
#ifndef BYOLO_H_
#define BYOLO_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BYOLO_API __attribute__((visibility("default")))

#define BYOLO_OK 0
#define BYOLO_ERR_ARG (-1)      /* invalid argument / graph construction error (reference: assert) */
#define BYOLO_ERR_STATE (-2)    /* call order violated (e.g. forward before finalize)             */
#define BYOLO_ERR_HIP (-3)      /* HIP runtime error                                              */
#define BYOLO_ERR_NOMEM (-4)    /* workspace too small                                            */
#define BYOLO_ERR_RANGE (-5)    /* split-f16 only: a value the reference's float32 tensors hold does not fit the
                                   hi/lo fp16 storage (|activation| > 16376), or a raw detection output is inf / NaN   */

typedef struct byolo byolo_t;

/* decode kinds == the three detection-layer factories of lib_yolo/model.py:107 / :132 / :157 */
enum { BYOLO_DET_STANDARD = 0, BYOLO_DET_ALEATORIC = 1, BYOLO_DET_EPISTEMIC = 2 };
/* inference_epistemic.py:99-102 (class-agnostic) and :104-126 (commented-out 2-class variant); BYOLO_NMS_PER_CLASS is that
 * variant for any class count: row i belongs to class c iff cls[i][c] > cls[i][k] for every k != c (float32, strictly: a
 * maximum attained twice or a NaN class score leaves the row in no class; with one class every row is in class 0), one
 * tf.image.non_max_suppression per class over its members, the kept rows of class 0, 1, ... back to back.  Two classes give
 * BYOLO_NMS_TWO_CLASS bit for bit, one class BYOLO_NMS_AGNOSTIC -- the three modes are ONE device pipeline that runs the
 * classes of an image side by side: BYOLO_NMS_AGNOSTIC is one class (every row whose score is a candidate; no class column is
 * read, the rows need not have any), BYOLO_NMS_TWO_CLASS two classes on the columns cls_start, cls_start + 1 (whatever the
 * handle's cls_cnt; byolo_forward insists on cls_cnt == 2).  Limits: 1 .. BYOLO_NMS_MAX_CLASSES classes (the class is one byte
 * above the score bits of the sort key, 255 = no class; the decode kernels stop at 128), N < 2^31 in every mode. */
enum { BYOLO_NMS_AGNOSTIC = 0, BYOLO_NMS_TWO_CLASS = 1, BYOLO_NMS_PER_CLASS = 2 };
#define BYOLO_NMS_MAX_CLASSES 128
/* normaliser list of lib_yolo/layers.py:556-571 */
enum { BYOLO_NORM_BN = 1, BYOLO_NORM_DROPOUT = 2 };

typedef struct byolo_cfg {
    int32_t img_h, img_w, img_c;  /* config['full_img_size'] (yolov3.py:207-208: h, w % 32 == 0)   */
    int32_t cls_cnt;              /* config['cls_cnt'], 1 .. 128                                    */
    float   drop_prob;            /* 0.1 hard-coded at lib_yolo/yolov3.py:462                       */
    int32_t max_out;              /* 1000: tf.image.non_max_suppression(.., 1000)                   */
    float   iou_thresh;           /* 0.5: TF default                                                */
    int32_t nms_mode;             /* BYOLO_NMS_*                                                    */
    int32_t keep_all_outputs;     /* 1 = no activation-buffer reuse, every layer readable (tests)   */
} byolo_cfg;

/* ---- lifetime ---------------------------------------------------------------------------- */
BYOLO_API int32_t byolo_create(const byolo_cfg* cfg, int32_t device, byolo_t** out);
BYOLO_API int32_t byolo_destroy(byolo_t* h);
/* Arithmetic of the convolution stack (the reference runs TensorFlow's float32 kernels, lib_yolo/layers.py:550; both
 * modes accumulate in fp32 and hold the 1e-4 contract against the float32 CPU restatement):
 *   BYOLO_PREC_F32        fp32 operands on the fp32 matrix instruction (v_mfma_f32_32x32x2_f32), Winograd F(2x2,3x3)
 *                         for the large 3x3 convolutions;
 *   BYOLO_PREC_SPLIT_F16  every activation / weight as hi + lo, two fp16 values (~23 significant bits), three fp16
 *                         matrix products per fp32 product into fp32 accumulators (v_mfma_f32_32x32x16_f16).  Weights
 *                         carry one exact power-of-two scale per OUTPUT CHANNEL (folded into the BN scale), so a filter
 *                         far smaller than its neighbours keeps its bits.  Activations are stored as 4 * value: one
 *                         beyond +-16376 does not fit -- that is DETECTED (byolo_status), never stored silently: see
 *                         BYOLO_ERR_RANGE and byolo_set_async below.
 * Default: environment BYOLO_PRECISION = f32 | split, else BYOLO_PREC_SPLIT_F16.  Call before byolo_finalize (a finalized
 * handle must be finalized again).  byolo_finalize itself falls back to BYOLO_PREC_F32 for a graph split storage cannot
 * express (a convolution whose output channels are not a multiple of 4 -- no reference model has one):
 * byolo_get_precision reports the mode in effect, byolo_precision_note why ("" if the request stands). */
enum { BYOLO_PREC_F32 = 0, BYOLO_PREC_SPLIT_F16 = 1 };
BYOLO_API int32_t byolo_set_precision(byolo_t* h, int32_t precision);
BYOLO_API int32_t byolo_get_precision(const byolo_t* h);
BYOLO_API const char* byolo_precision_note(const byolo_t* h);
BYOLO_API const char* byolo_last_error(const byolo_t* h);
BYOLO_API const char* byolo_version(void);
/* Incremented on every incompatible change of a signature or of a buffer layout this header describes, so that a binding can
 * refuse a library it was not written for (byolo/_lib.py does).  4: byolo_forward takes d_mask_bits; detection rows handed out
 * by byolo_layer_output are padded to a multiple of 4 floats; the host-side feed / writer entry points exist.  5: byolo_encode_gt,
 * byolo_loss (ground-truth encoding and training loss) exist.  6: the dropout stream byolo_forward draws from `seed` is redefined
 * (one hash + one derived word per group of four channels, csrc/byolo_rng.h): the same seed gives other masks than ABI 5 did; the
 * bit order of injected masks (d_mask_bits) is unchanged.  7: the plan of a handle is part of the ABI (byolo_plan_opts, byolo_get_plan_opts /
 * byolo_set_plan_opts, byolo_graph_stats): the BYOLO_* plan variables are read ONCE, at byolo_create, and no longer reach an existing
 * handle; a drop_prob whose 16-bit threshold rounds to 2^16 (rate 0) is the identity. */
#define BYOLO_ABI_VERSION 7
BYOLO_API int32_t byolo_abi_version(void);

/* ---- the plan of a handle: which kernel carries which layer, and how a forward is put on the stream -------------------------------
 * The reference leaves all of this to TensorFlow's placer and kernel registry (`sess.run`, inference_epistemic.py:76); here it is a
 * per-HANDLE struct, so that two handles in one process may differ and nothing outside a handle steers it.  byolo_create fills it
 * with the defaults below and then applies the environment variables named in brackets (the A/B switches of tools/ and tests/;
 * read ONCE, at byolo_create, never again); byolo_set_plan_opts replaces it.  Fields marked [pack] change what byolo_finalize packs:
 * set them before byolo_finalize (a finalized handle is marked un-finalized when one of them changes); the others may change between
 * forwards (the next forward plans again).  Every setting computes the layer functions of lib_yolo/layers.py:545-575; settings that
 * change the order of a floating-point sum (split-K, stream-K, Winograd on / off) change results within the fp32 re-association
 * error, all others bit for bit -- tests/test_gpu_parity.py holds each of them to the oracle. */
typedef struct byolo_plan_opts {
    int32_t struct_bytes;          /* sizeof(byolo_plan_opts) of the caller's header: a mismatch is BYOLO_ERR_ARG                      */
    int32_t graphs;                /* launch-graph replay of a whole forward: 0 never, 1 forwards that do not fill the chip by
                                      themselves (< 1 TFLOP: detect.py's batch-1 loop, BASELINE configs[0..1]; default), 2 every forward
                                      that can be captured [BYOLO_GRAPHS]                                                             */
    int32_t serialize_convs;       /* forwards of one handle on several streams: convolution stacks one after the other: 0 never,
                                      1 forwards of >= 1 TFLOP (default), 2 always [BYOLO_SERIALIZE_CONVS]                            */
    int32_t serialize_heads;       /* with serialize_convs in effect: only the HEADS wait for the other stream's convolution stack; this
                                      forward's backbone (small launches that leave CUs idle) runs beside the previous forward's heads: 1
                                      (default; +1.8 % img/s at configs[3]), 0 = the whole stack waits.  A forward recorded at profiling
                                      level 2 and the one after it always wait as a whole [BYOLO_SERIALIZE_HEADS]                      */
    int32_t dedup;                 /* [pack] T-invariant de-duplication (a convolution over a T-fold tile runs once per image): 1
                                      [BYOLO_NO_DEDUP inverts]                                                                        */
    int32_t lowmain;               /* [pack] the 1x1 convolution over an upsampled source at the source's resolution: 1 [BYOLO_LOWMAIN] */
    int32_t kx3, p1;               /* [pack] split-f16 K loops: shared-tap 3x3 stages / uniform 1x1 loop: 1, 1 [BYOLO_KX3, BYOLO_P1]   */
    int32_t b2b;                   /* 3x3 + following 1x1 in one launch (76x76 head pairs): 0 never, 1 launches of >= 4 rounds
                                      (default), 2 every eligible pair [BYOLO_B2B]                                                    */
    int32_t kx3_wide;              /* the 8-wave 128 x 256 shared-tap tile without a follower: 0 (default; measured 4 % slower), 1, 2
                                      [BYOLO_KX3_WIDE]                                                                                */
    int32_t wino_split;            /* Winograd F(2x2,3x3) in split-f16: 0 never, 1 the layers with >= wino_split_min_c input channels the
                                      planner's time model (byolo_plan.hip) expects >= 3 % faster than the direct kernel (default),
                                      2 every eligible layer [BYOLO_WINO_SPLIT]                                                       */
    int32_t wino_split_min_c;      /* 256 [BYOLO_WINO_SPLIT_MIN_C]                                                                    */
    int32_t wino_split_bn;         /* output channels per workgroup: 0 the time model picks per layer (default: 256 for launches of
                                      many rounds, 128 where that fills more CUs), 256 (8 waves) or 128 forced [BYOLO_WINO_SPLIT_BN]  */
    int32_t wino_split_rounds;     /* experiment: chunks of k whole rounds of workgroups, 0 = off [BYOLO_WINO_SPLIT_ROUNDS]           */
    int32_t winograd;              /* fp32 mode: Winograd for the large 3x3 layers: 0, 1 (default), 2 every eligible [BYOLO_WINOGRAD] */
    int32_t wino_fused;            /* fp32 mode: GEMM + output transform in one kernel: 0, 1 (default), 2 [BYOLO_WINO_FUSED]          */
    int32_t stream1x1;             /* fp32 mode: row-streaming 1x1 launches: 0, 1 (default), 2 [BYOLO_STREAM1X1]                      */
    int32_t gemm_stream;           /* fp32 mode: the unfused Winograd GEMM on the row-streaming kernel: 1 [BYOLO_GEMM_STREAM]         */
    int32_t ksplit;                /* split-K of a launch's last partial round: -1 the cost model (default), 0 never, n > 1 always n
                                      slices [BYOLO_KSPLIT]                                                                           */
    int32_t streamk;               /* stream-K for small launches: 0 never, 1 the cost model (default), 2 whenever admissible
                                      [BYOLO_STREAMK]                                                                                 */
    int32_t plain_epilogue;        /* straight-line epilogues of the split-f16 convolutions (one decision per tile): 1; 0 = the general
                                      epilogue everywhere (A/B; the same bits) [BYOLO_PLAIN_EPILOGUE]                                 */
    int32_t wshift_per_layer;      /* [pack] split-f16 weights: ONE power-of-two scale per layer instead of one per output channel: 0; 1 = the
                                      A/B of tests/test_robustness.py (a filter far smaller than its neighbours loses bits)
                                      [BYOLO_WSHIFT_PER_LAYER]                                                                        */
    int32_t nms_general;           /* the tail's general path (sort + bit-matrix NMS over all candidates) for every image, never the
                                      top-k fast path: 0; 1 = tests / soak runs of that path [BYOLO_NMS_GENERAL]                      */
    int32_t wino_split_persist;    /* the Winograd GEMM's workgroups walk the unit list themselves, next unit prefetched: 0 one unit per
                                      workgroup (default), 1 a static list, 2 units claimed from a per-XCD counter; the same bits, and
                                      measured SLOWER: +2.5 % / +0.8 % per launch (profiles/r6_wino_persist.md) [BYOLO_WINO_SPLIT_PERSIST] */
    int32_t wino_split_feed;       /* the split-f16 Winograd input transform evaluates the element-wise pass in front of it itself, when it
                                      is that pass's only reader: bit 0 = the T-fold replay of a per-image convolution's epilogue (that
                                      convolution then stores raw accumulators once per image), bit 1 = the finish of a 1x1 convolution
                                      over an upsampled source (that launch is not issued); the tensor in between gets no memory.  3
                                      (default), 0 = the two-launch plan; the same bits (profiles/wino_feed.md) [BYOLO_WINO_SPLIT_FEED]  */
    float   wino_split_min_gflop;  /* a floor under the time model: 30 [BYOLO_WINO_SPLIT_MIN_GFLOP]                                   */
    float   wino_split_chunk_mb;   /* V bytes of one chunk: 1500 [BYOLO_WINO_SPLIT_CHUNK_MB]                                          */
    float   wino_min_gflop;        /* fp32 mode: 10 [BYOLO_WINO_MIN_GFLOP]                                                            */
    float   wino_chunk_mb;         /* fp32 mode: V + M bytes of one chunk: 800 [BYOLO_WINO_CHUNK_MB]                                  */
    float   wino_min_ratio;        /* fp32 mode: Cin * cout / (Cin + cout) at least: 80 [BYOLO_WINO_MIN_RATIO]                        */
} byolo_plan_opts;
BYOLO_API int32_t byolo_get_plan_opts(const byolo_t* h, byolo_plan_opts* out);       /* out->struct_bytes is set                     */
BYOLO_API int32_t byolo_set_plan_opts(byolo_t* h, const byolo_plan_opts* opts);
/* Launch graphs kept by the handle (one per distinct argument set of a replayed forward; at most 8, least recently used dropped) and
 * how often a forward was replayed / captured / updated in place (a forward whose dropout seed differs from the captured one). */
BYOLO_API int32_t byolo_graph_stats(const byolo_t* h, int32_t* n_graphs, int64_t* replays, int64_t* captures, int64_t* updates);

/* ---- graph construction: one call per ModelBuilder.make_* (lib_yolo/model.py:52-185).
 * Each returns the new layer's index (>= 0) in the reference's `ModelBuilder.__layers` numbering
 * (model.py:40-41) or a negative error.  Layer references (`shortcut`, `routes`, `src`) follow
 * the reference: negative = relative to the end of the list, non-negative = absolute.
 *
 *
 * Route / upsample / stack layers are VIEWS: they exist only inside the loader of the convolution that reads them
 * (two concatenated sources, each upsampled at most once), and a residual add rides in the epilogue of the
 * convolution in front of it.  That covers everything the reference's three models build at no cost.  A general
 * ModelBuilder graph is accepted as well; what does not fit is lowered to plain steps of its own:
 *   - the inner view of a nested concat / double upsample, or a view used as an operand of a residual add, is
 *     copied into a tensor first;
 *   - a residual add whose left operand is not a convolution, or whose convolution has other readers, runs as an
 *     element-wise kernel;
 *   - input channels that are not a multiple of 32 (per concatenated source) take a general direct convolution
 *     instead of the matrix-pipe one -- correct, slow. ---------------------------------------------------------- */

/* make_conv_layer / make_downsample_layer / make_darknet_conv_layer / make_darknet_downsample_layer
 * (model.py:52-81 -> layers.conv, lib_yolo/layers.py:545-575): conv(no bias) -> [dropout] -> BN
 * (eps 1e-5) -> leaky-ReLU(0.1).  stride 2 = pad(1,1)+VALID (layers.py:533-537, :616-635).
 * `scope` = TF variable scope of the layer ("darknet53/conv_3", ...): names its variables
 * "<scope>/conv2d/kernel", "<scope>/batch_normalization/{gamma,beta,moving_mean,moving_variance}".
 * At most 65 536 filters and 2^28 weights per kernel (the reference's largest: 1024 / 4.7 M): beyond, BYOLO_ERR_ARG.
 * No entry point lets a C++ exception out: a host allocation that fails is BYOLO_ERR_NOMEM. */
BYOLO_API int32_t byolo_add_conv(byolo_t* h, const char* scope, int32_t filters, int32_t ksize, int32_t stride,
                       int32_t norm_flags);
/* make_residual_layer (model.py:91-94, layers.py:505-507) */
BYOLO_API int32_t byolo_add_residual(byolo_t* h, int32_t shortcut);
/* make_route_layer (model.py:83-86, layers.py:583-592): 1 route = identity, 2 = channel concat */
BYOLO_API int32_t byolo_add_route(byolo_t* h, const int32_t* routes, int32_t n_routes);
/* make_upsample_layer (model.py:101-105, layers.py:578-580): nearest x2 */
BYOLO_API int32_t byolo_add_upsample(byolo_t* h);
/* make_stack_feature_map_layer (model.py:88-89, layers.py:595-597): tile T x on the batch axis;
 * T is a run-time argument of byolo_forward.  Sample order: s = img*T + t. */
BYOLO_API int32_t byolo_add_stack(byolo_t* h, int32_t src);
/* make_detection_layer{,_aleatoric,_aleatoric_epistemic} (model.py:107-185): 1x1 conv + bias,
 * linear (layers.py:600-613), then split + decode (layers.py:11-84, :191-502).  priors_hw = the 3
 * (h, w) priors of this stride; layer_id = len(det_layers) so far (model.py:141, :167). */
BYOLO_API int32_t byolo_add_detection(byolo_t* h, const char* scope, int32_t kind, const float* priors_hw /*[3][2]*/);

/* `self.__darknet53_layer_cnt = mb.layer_cnt()` (lib_yolo/yolov3.py:246): everything added so far
 * is the backbone (used for load_darknet53_weights and for the per-stage timers). */
BYOLO_API int32_t byolo_mark_backbone_end(byolo_t* h);

/* ---- parameters: tf.train.Saver.restore / darknet.load_darknet_weights
 * (inference_epistemic.py:58, lib_yolo/darknet.py:42-122) ------------------------------------ */
BYOLO_API int32_t byolo_num_params(const byolo_t* h);
BYOLO_API int32_t byolo_param_info(const byolo_t* h, int32_t i, const char** name, int32_t* ndim, int64_t shape[4]);
BYOLO_API int32_t byolo_set_param(byolo_t* h, const char* name, const float* h_data, int64_t count);
BYOLO_API int32_t byolo_get_param(const byolo_t* h, const char* name, float* h_data, int64_t count);
/* fold BN (+ 1/keep_prob) into per-channel scale/shift, repack kernels for the MFMA tiles, upload.
 * May be called again after further byolo_set_param calls.  Packs on the host's cores (environment
 * BYOLO_FINALIZE_THREADS: default the hardware threads / LOCAL_WORLD_SIZE -- one process per GPU, the ranks of a node finalize
 * together --, at most 32; the packed bytes do not depend on it). */
BYOLO_API int32_t byolo_finalize(byolo_t* h);

/* ---- run: one sess.run([nms_op]) (inference_epistemic.py:76, inference_aleatoric.py:75) ------ */
BYOLO_API int32_t byolo_num_layers(const byolo_t* h);
BYOLO_API int32_t byolo_num_boxes(const byolo_t* h, int64_t* n_boxes, int32_t* row_len);   /* N, D of concat_bbox */
BYOLO_API int32_t byolo_workspace_bytes(byolo_t* h, int32_t B, int32_t T, size_t* out);
/* Introspection of the workspace plan of a (B, T) call, host only (no device, no byolo_finalize needed) -- what tests/test_planner.py
 * checks on the CPU: no tensor is written while another tensor that shares its memory is still to be read.
 *   byolo_plan_num     makes the plan (inject != 0: the plan of a call with d_mask_bits); steps, tensors, arena size;
 *   byolo_plan_step    the tensor step `step` writes; fuses_next = 1 when step + 1 runs INSIDE this step's launch (its output is
 *                      written during this step, this step's own output tensor never exists); the tensors the step's launch reads;
 *                      a step folded into its reader's Winograd input transform (wino_split_feed) reports what it really leaves in
 *                      memory -- the per-image raw accumulators (an auxiliary tensor), or, launching nothing, the low-resolution
 *                      operand it hands on -- and that reader reports those operands as what it reads;
 *   byolo_plan_tensor  offset in the workspace (< 0: none in this plan), size, and whether anything reads it after the last step
 *                      (a detection layer's raw output: the decode launch; every layer under keep_all_outputs). */
BYOLO_API int32_t byolo_plan_num(byolo_t* h, int32_t B, int32_t T, int32_t inject, int32_t* n_steps, int32_t* n_tensors, int64_t* arena_bytes);
BYOLO_API int32_t byolo_plan_step(byolo_t* h, int32_t step, int32_t* out_tensor, int32_t* fuses_next, int32_t reads[8], int32_t* n_reads);
BYOLO_API int32_t byolo_plan_tensor(byolo_t* h, int32_t tensor, int64_t* offset, int64_t* bytes, int32_t* read_after_the_steps);
/* d_img [B,H,W,C] NHWC fp32.  T = MC samples (1 for graphs without stack layers).
 * Outputs (any may be NULL to skip that stage's export):
 *   d_boxes   [B,N,D]               pre-NMS rows in concat_bbox order (inference_*.py concat_bbox)
 *   d_rows    [B,max_out*(1|2),D]   NMS-kept rows, score order (2-class: ped rows then rider rows)
 *   d_kept    [B,max_out*(1|2)]     int32 global box indices of the kept rows
 *   d_count   [B,2]                 int32 {total kept, kept in first class (== total if agnostic)}
 *   BYOLO_NMS_PER_CLASS: d_rows [B,cls_cnt*max_out,D], d_kept [B,cls_cnt*max_out] (class 0's kept rows, then class 1's, ...;
 *   zero rows / -1 behind the last), d_count as above; the kept-per-class counts [B,cls_cnt]: byolo_nms_class_counts.
 * seed: dropout stream (see csrc/byolo_rng.h); dropout is active iff the layer has
 * BYOLO_NORM_DROPOUT and `dropout_on` != 0 (standard_test_dropout=True quirk, layers.py:567-568).
 * d_mask_bits (nullable): INJECTED dropout masks instead of the library's counter stream -- tf.layers.dropout draws
 *   its Bernoulli noise from an unseeded op (layers.py:521-524), so a caller that wants the reference's masks (or its
 *   own) passes them: one bit per element of each dropout layer's input [S,h,w,cout] of THIS call (S = B*T in the
 *   stacked part of the graph; byolo_set_first_image does not enter), 1 = keep, layer after layer at the bit offsets of
 *   byolo_mask_layout.
 * Numeric status (split precision): unless byolo_set_async(h, 1), the call waits for the stream and returns
 *   BYOLO_ERR_RANGE -- never rows of inf / NaN -- when an activation left the split-f16 range; outputs are then undefined.
 * Any B: a batch beyond byolo_max_images(h, T) runs inside this call as consecutive pieces of at most that many images in the
 *   same workspace (byolo_workspace_bytes sizes it for the largest piece), each drawing the dropout masks of its position in
 *   the batch -- the result does not depend on the cut (images are independent; the NMS is per image).  Injected masks
 *   (d_mask_bits) describe one piece: with them B must not exceed byolo_max_images.  byolo_layer_output then shows the LAST piece. */
BYOLO_API int32_t byolo_forward(byolo_t* h, const float* d_img, int32_t B, int32_t T, uint64_t seed, int32_t dropout_on,
                      const uint32_t* d_mask_bits, void* d_workspace, size_t workspace_bytes,
                      float* d_boxes, float* d_rows, int32_t* d_kept, int32_t* d_count, void* stream);
/* Dropout layers of the graph (creation order = the `ordinal` of csrc/byolo_rng.h), and where layer `ordinal`'s bits sit in
 * d_mask_bits for a (B, T) call: bit_offset (a multiple of 32) and element count S*h*w*cout; ordinal == byolo_num_dropout
 * returns the total length in bits (a multiple of 32) in bit_offset. */
BYOLO_API int32_t byolo_num_dropout(const byolo_t* h);
BYOLO_API int32_t byolo_mask_layout(byolo_t* h, int32_t B, int32_t T, int32_t ordinal, int64_t* bit_offset, int64_t* elements);
/* Numeric status of the handle's forwards in BYOLO_PREC_SPLIT_F16.  Every epilogue that encodes an activation tracks the
 * largest magnitude it stores, every decode launch checks the raw detection outputs; a hit raises a sticky device word:
 *   flags bit 0  an activation beyond the split-f16 range in layer `layer` (the first such layer; -1 otherwise)
 *   flags bit 1  a raw detection output is inf / NaN
 * byolo_status WAITS for `stream`, returns BYOLO_OK or BYOLO_ERR_RANGE (message: the layer's scope) and leaves the words
 * set; byolo_clear_status resets them (asynchronously, on `stream`).  byolo_set_async(h, 1): byolo_forward no longer waits
 * and checks -- a caller that synchronises anyway (to copy rows to the host) asks byolo_status once there.  Default 0. */
BYOLO_API int32_t byolo_set_async(byolo_t* h, int32_t on);
BYOLO_API int32_t byolo_status(byolo_t* h, void* stream, uint32_t* flags, int32_t* layer);
BYOLO_API int32_t byolo_clear_status(byolo_t* h, void* stream);
/* The dropout stream is indexed by the element index in the [S,h,w,c] tensor, S = images*T.  When one logical
 * batch is processed in several calls (sub-batches that respect byolo_max_images, or one shard per GPU), tell
 * every call where its first image sits in the logical batch: image j of the call then draws the masks of image
 * first_image + j, and the pieces equal the unsplit run.  Sticky per handle; 0 after byolo_create. */
BYOLO_API int32_t byolo_set_first_image(byolo_t* h, int64_t first_image);
/* T sharded over ranks -- the latency path for the reference's own default, ONE image per step (inference_epistemic.py:193
 * asserts batch_size == 1, :220 T = 50), where sharding the batch axis leaves N - 1 GPUs idle (the alternative):
 * every rank runs the backbone on the image and the heads on T_local = its share of the T_total MC samples.
 *   byolo_set_tshard(h, t0, T_total)   sticky; T_total = 0 switches it off.  A following byolo_forward(h, img, B = 1, T = T_local,
 *       ...) draws the dropout masks of samples t0 .. t0 + T_local - 1 of the image's T_total (the N ranks together draw what one
 *       call with T = T_total draws) and writes into d_boxes [B, N, 21 + C], instead of decoded rows, the per-box SUMS over its
 *       samples of the quantities lib_yolo/layers.py:377-395 reduces with reduce_mean: [sum l (4) | sum l l^T, upper triangle (10) |
 *       sum exp(logvar) (4) | sum sigmoid(obj) | sum H(sigmoid(obj)) | sum softmax(cls) (C) | sum H(softmax(cls))].  d_rows must be
 *       null (no NMS on sums).  Epistemic detection layers only.
 *   the caller adds the ranks' buffers element-wise (one all-reduce of N * (21 + C) floats: 2.1 MB at 608 x 608);
 *   byolo_finish_tshard(h, d_sums, B, T_total, stream)   turns the summed buffer IN PLACE into the rows a T_total-sample
 *       byolo_forward writes (means, population covariance, 4x4 determinant, entropies / mutual information, decoded corners);
 *       byolo_sort_nms then runs the tail.  The sums are added in another order than the one-call reduction: rows agree within
 *       float32 rounding (tested at the contract's bound 1e-4 * max(1, |ref|)), not bit for bit. */
BYOLO_API int32_t byolo_set_tshard(byolo_t* h, int32_t t0, int32_t T_total);
BYOLO_API int32_t byolo_finish_tshard(byolo_t* h, float* d_sums, int32_t B, int32_t T_total, void* stream);
/* Images ONE launch sequence carries at this T: the convolutions address their sources with 32-bit byte offsets, so every
 * activation tensor [B*T or B, h, w, c] of a piece stays below 3 GiB (18 images at 608x608, T=30).  byolo_forward cuts larger
 * batches into such pieces itself; the number matters to a caller that injects masks or reads byolo_layer_output. */
BYOLO_API int32_t byolo_max_images(byolo_t* h, int32_t T, int32_t* max_images);
/* After a forward with keep_all_outputs: device pointer + NHWC shape of layer `idx`'s output
 * (the reference's model.layers[idx], model.py:191); for detection layers the raw conv output
 * (DetLayer.raw_output, model.py:241) -- those are readable on any handle (they are never overwritten).
 * The pointer addresses the library's own storage: hi/lo pairs under BYOLO_PREC_SPLIT_F16, and a detection head's rows
 * are padded to a multiple of 4 floats (shape[3] = 21 / 42 / .. is the logical count): read tensors through
 * byolo_copy_layer_output, which hands out dense float32. */
BYOLO_API int32_t byolo_layer_output(const byolo_t* h, int32_t idx, const float** d_ptr, int64_t shape[4]);
/* The same tensor as float32 values, copied into caller-owned device memory d_dst[count] (count = the product of the
 * shape) on `stream`.  Under BYOLO_PREC_SPLIT_F16 the pointer of byolo_layer_output addresses the hi/lo pairs the
 * kernels exchange (only detection layers are plain float32 there): read activations through this call. */
BYOLO_API int32_t byolo_copy_layer_output(const byolo_t* h, int32_t idx, float* d_dst, int64_t count, void* stream);

/* ---- staged tail entry points (parity tests on oracle-provided inputs) ------------------------ */
/* decode one detection layer: d_raw [S,lh,lw,F] -> rows written at their concat_bbox position in
 * d_boxes [B,N_total,D] starting at box offset `box_base` (d_raw dense, F floats per cell); kind as above; EPISTEMIC reduces every
 * image's T samples (S = B*T). */
BYOLO_API int32_t byolo_decode(byolo_t* h, int32_t kind, const float* d_raw, int32_t B, int32_t T, int32_t lh, int32_t lw,
                     const float* priors_hw /*[3][2] host*/, int32_t layer_id, float* d_boxes,
                     int64_t n_total, int64_t box_base, void* stream);
/* The entries of decode_epistemic's dict (lib_yolo/layers.py:397-411) that are not columns of the box row, from the
 * raw output d_raw [B*T,lh,lw,3*2*(5+C)] of an epistemic detection layer, DENSE float32 (as byolo_copy_layer_output hands it
 * out; the library's own storage pads the rows, see byolo_layer_output): ev_loc [B,lh,lw,3,4]
 * (mean raw location logits), epi_covar_loc [B,lh,lw,3,4,4] (full covariance; its diagonal is columns 4..7 of the box
 * row), obj_samples [B*T,lh,lw,3] = sigmoid(obj), cls_samples [B*T,lh,lw,3,C] = softmax(cls).  Any output may be NULL.
 * (vis_uncertainty.py:49-163 and other consumers of DetLayer.det.) */
BYOLO_API int32_t byolo_epistemic_stats(byolo_t* h, const float* d_raw, int32_t B, int32_t T, int32_t lh, int32_t lw,
                                        float* d_ev_loc, float* d_epi_covar, float* d_obj_samples, float* d_cls_samples,
                                        void* stream);
/* ---- MC sample-count ladder: the epistemic rows at several sample counts T from ONE forward ----
 * The epistemic decode walks an image's T samples in order with running sums; the sums after k samples are what a T = k
 * reduction of the image's first k samples holds.  One pass over the raw detection outputs therefore finishes the rows at every
 * "rung" of a ladder of sample counts: rungs[0] < rungs[1] < ... , each in 1 .. T, at most BYOLO_T_LADDER_MAX of them; rung k's
 * rows fill slab k of d_boxes [n_rungs][B][N][21+C].  Models of at most BYOLO_T_LADDER_MAX_CLASSES classes (the builds of the
 * ladder kernel that keep their per-lane state in registers; more is refused with BYOLO_ERR_ARG).
 *   byolo_decode_ladder   staged, one detection layer: like byolo_decode(kind = EPISTEMIC, ...), d_raw dense
 *       [B*T, lh, lw, 3*2*(5+C)]; the layer's rows of rung k go to slab k at box offset box_base, nothing else is written.
 *   byolo_forward_ladder  the LAST forward's raw detection outputs, every detection layer -> d_boxes [n_rungs][B][N][D]; with a
 *       variance recalibration set on the handle (byolo_set_var_recal) every slab is recalibrated in place as a forward's rows
 *       are, so a slab is what a forward would hand the NMS.
 * What is promised: rung k is the existing decode of THIS forward's first k samples of every image, bit for bit (the slab of
 * rung T equals the forward's own d_boxes).  Those samples are independent draws like any other k.
 * What is NOT promised: that rung k equals a separate byolo_forward(T = k).  The per-layer plan (split-K, stream-K, the Winograd
 * choice) depends on B*T and changes the order of summation, and for images after the first the dropout element index depends
 * on T (see byolo_set_first_image), so such a forward draws other masks.
 * Ordering: the call reads the workspace of the forward it follows.  It must be ordered on `stream` BEHIND that forward, and
 * come BEFORE the next forward into the same workspace; it launches on `stream` and does not wait.
 * BYOLO_ERR_STATE: no forward has run (or the plan is not valid).  BYOLO_ERR_ARG, before anything is launched: B or T are not
 * the last forward's (this includes a batch beyond byolo_max_images, which ran in pieces), a T shard is set (byolo_set_tshard),
 * a detection layer that is not epistemic or not stacked, no rungs, more than BYOLO_T_LADDER_MAX, rungs that are not strictly
 * increasing or lie outside 1 .. T, more classes than the limit. */
#define BYOLO_T_LADDER_MAX 16
#define BYOLO_T_LADDER_MAX_CLASSES 48
BYOLO_API int32_t byolo_decode_ladder(byolo_t* h, const float* d_raw, int32_t B, int32_t T, int32_t lh, int32_t lw,
                            const float* priors_hw /*[3][2] host*/, int32_t layer_id, const int32_t* rungs /*host*/, int32_t n_rungs,
                            float* d_boxes, int64_t n_total, int64_t box_base, void* stream);
BYOLO_API int32_t byolo_forward_ladder(byolo_t* h, int32_t B, int32_t T, const int32_t* rungs /*host*/, int32_t n_rungs,
                             float* d_boxes, void* stream);
/* tf.image.non_max_suppression + tf.gather per image on d_boxes [B,N,D] (scores = column obj_idx).
 * Visiting order: descending score, the lower row index first among equal scores.  Equal is the float32 comparison: -0.0 and
 * +0.0 are one score and their rows are ordered by index alone.  A NaN score or one <= -FLT_MAX is no candidate.
 * d_sort_ws: >= byolo_nms_workspace_bytes(B, N), the size of two classes, enough for BYOLO_NMS_AGNOSTIC and BYOLO_NMS_TWO_CLASS;
 * BYOLO_NMS_PER_CLASS: >= byolo_nms_workspace_bytes_ex(B, N, nms_mode, cls_cnt) (the other modes: the same value as
 * byolo_nms_workspace_bytes; 0 for arguments the mode refuses).  BYOLO_NMS_AGNOSTIC ignores cls_start_idx.  The per-class mode takes
 * its class count from the handle (byolo_cfg.cls_cnt), reads the class scores in columns cls_start_idx .. cls_start_idx +
 * cls_cnt - 1 and sizes d_rows / d_kept by cls_cnt * max_out per image (see byolo_forward).  Refused with BYOLO_ERR_ARG before
 * anything is launched: an unknown mode, class columns outside the row, max_out above 2048 (the limit PER CLASS).
 * byolo_nms_class_counts: the kept-per-class counts [B,cls_cnt] int32 of the handle's LAST per-class NMS (byolo_sort_nms or
 * byolo_forward with d_rows), copied to d_class_counts on `stream` (order it behind that call); B and cls_cnt must be that
 * call's.  BYOLO_ERR_STATE before the first such call. */
BYOLO_API size_t  byolo_nms_workspace_bytes(int32_t B, int64_t N);
BYOLO_API size_t  byolo_nms_workspace_bytes_ex(int32_t B, int64_t N, int32_t nms_mode, int32_t cls_cnt);
BYOLO_API int32_t byolo_nms_class_counts(byolo_t* h, int32_t* d_class_counts, int32_t B, int32_t cls_cnt, void* stream);
BYOLO_API int32_t byolo_sort_nms(byolo_t* h, const float* d_boxes, int32_t B, int64_t N, int32_t D, int32_t obj_idx,
                       int32_t cls_start_idx, int32_t nms_mode, int32_t max_out, float iou_thresh,
                       void* d_sort_ws, size_t ws_bytes,
                       float* d_rows, int32_t* d_kept, int32_t* d_count, void* stream);

/* ---- ground-truth encoding and training loss ------------------------
 * The reference builds both into its TRAINING graph; here they are two stand-alone device functions (the optimiser, batch-
 * statistics BN and back-propagation through the network stay out of scope).  `h` supplies the device and the error string
 * and may be NULL (current device, byolo_last_error(NULL)).
 *
 * byolo_encode_gt = lib_yolo/tfdata.py:77-171 `encode_boxes` (the map function of the training dataset,
 * lib_yolo/dataset_utils.py:58-63) for a batch of B images: boxes [B,max_boxes,4] as (ymin, xmin, ymax, xmax) image
 * fractions, labels [B,max_boxes], counts [B] (NULL: every image has max_boxes boxes); detection layers as
 * layer_hw [n_layers][2] and priors_hw [n_layers][3][2] = (h, w) DOUBLES (the Python floats of lib_yolo/yolov3.py:6-166: the
 * prior boxes are computed in double and rounded to float32 like lib_yolo/data.py:125-166 does).  Outputs, per image the prior
 * boxes of all layers back to back, inside a layer in the reference's [row, col, box] order (N = sum of lh * lw * 3): loc [B,N,4]
 * (logit / log targets), obj [B,N], cls [B,N] (int32), ign [B,N]; layer k's slice reshapes to the reference's
 * gt_k['loc'] [lh,lw,3,4] etc.  Later boxes overwrite earlier ones that claim the same prior box, as the reference's
 * sequential tf.while_loop does.  The masks are bit-identical to a float32 evaluation of the reference's formulas.  d_boxes 16-byte
 * aligned; d_workspace >= byolo_encode_gt_workspace_bytes(B, max_boxes) (every box's maximum IoU over all prior boxes). */
BYOLO_API int32_t byolo_encode_gt(byolo_t* h, int32_t n_layers, const int32_t* layer_hw, const double* priors_hw,
                                  const float* d_boxes, const int32_t* d_labels, const int32_t* d_counts, int32_t B,
                                  int32_t max_boxes, float ign_thresh, float* d_loc, float* d_obj, int32_t* d_cls,
                                  float* d_ign, void* d_workspace, size_t workspace_bytes, void* stream);
BYOLO_API size_t  byolo_encode_gt_workspace_bytes(int32_t B, int32_t max_boxes);
/* byolo_loss = lib_yolo/layers.py:126-188 `loss_tf` for ONE detection layer on its raw output d_raw [S,lh,lw,pitch]
 * (pitch = floats per cell, 0 = dense; the library's own storage pads, see byolo_layer_output), split as
 * lib_yolo/layers.py:11-84 does: kind BYOLO_DET_STANDARD (loc 4, obj, cls C per prior) or BYOLO_DET_ALEATORIC (loc 4,
 * log_loc_var 4, obj, log_obj_stddev, cls C, log_cls_stddev C); aleatoric_loss as the reference's flag (lib_yolo/layers.py:150-153,
 * log variance clipped to [-40, 40]).  Ground truth as byolo_encode_gt lays it out: pointers at the layer's first prior box,
 * gt_stride = prior boxes between consecutive images (N of byolo_encode_gt, or lh * lw * 3 for per-layer arrays).
 * d_loss[3] (double) = loc, obj, cls: sum / (2 S), sum / S, sum / S.  d_grad (or NULL) [S,lh,lw,grad_pitch] receives
 * d(loc + obj + cls) / d(raw) -- what lib_yolo/train.py:88 `optimizer.minimize` would send into the network.  Terms are
 * float32 like the graph's, sums double in a fixed order: results are deterministic.  d_workspace >= byolo_loss_workspace_bytes(). */
BYOLO_API size_t  byolo_loss_workspace_bytes(void);
BYOLO_API int32_t byolo_loss(byolo_t* h, int32_t kind, int32_t aleatoric_loss, int32_t cls_cnt, const float* d_raw, int32_t pitch,
                             int32_t S, int32_t lh, int32_t lw, const float* d_gt_loc, const float* d_gt_obj,
                             const int32_t* d_gt_cls, const float* d_gt_ign, int64_t gt_stride, double* d_loss,
                             float* d_grad, int32_t grad_pitch, void* d_workspace, size_t workspace_bytes, void* stream);

/* ---- synthetic-weight support: data-dependent BN initialisation (no reference counterpart;
 * replaces "train the network" for benchmarking with random-init weights): runs the graph on
 * d_img with dropout off, sets every BN's moving_mean/variance to the batch statistics of its conv
 * output layer by layer, re-folds.  Read the result back with byolo_get_param.
 * The contract (tests/test_calibrate_gpu.py, against oracle/cpu_ref.forward(calibrate=True) in float64; measured distances in
 * profiles/calibrate_parity.md):
 *   - the statistics of a layer are those of its RAW convolution output (before dropout, BN and leaky-ReLU) over all B * h * w rows,
 *     computed on the activations the layers in front produce with the statistics just set for them;
 *   - the variance is the biased one (divided by the row count, like tf.nn.moments);
 *   - dropout is off; a stacked graph runs at T = 1;
 *   - sums are accumulated in double, around the channel's value in row 0, in a fixed order: a channel of mean 1000 and variance
 *     1e-6 comes out to 1e-4 relative, one row gives variance exactly 0, and the result is deterministic (calibrating twice, or two
 *     handles on the same frames, gives identical parameters);
 *   - in every precision and plan the handle afterwards equals one finalized from byolo_get_param's values: a forward on either gives
 *     the same bits; launch graphs captured before the call replay with the new statistics; with keep_all_outputs,
 *     byolo_layer_output reads the (B, T = 1) run the calibration left in d_workspace.
 * Frames that give fewer than about 9 rows at the coarsest grid (B * h * w at stride 32) produce near-zero variances: the folded
 * 1 / sqrt(var + 1e-5) then amplifies rounding by up to 316 per layer and the weights are ill conditioned.  Statistics that are
 * not finite are BYOLO_ERR_ARG.  BYOLO_PREC_SPLIT_F16: the activations the call stores are range-checked like a forward's -- one
 * beyond |v| < 16380 (the image included) ends the call with BYOLO_ERR_RANGE naming the layer, its statistics already set, the
 * layers behind it untouched and the status words cleared; words an asynchronous forward left raised are reported first, the same way. */
BYOLO_API int32_t byolo_calibrate_bn(byolo_t* h, const float* d_img, int32_t B, void* d_workspace, size_t workspace_bytes,
                           void* stream);

/* ---- profiling hooks: per-stage device time of the LAST forward (hipEvents on `stream`);
 * enable with byolo_set_profiling(h, 1).  stage: 0 backbone, 1 heads, 2 decode, 3 sort+nms. */
BYOLO_API int32_t byolo_set_profiling(byolo_t* h, int32_t on);   /* 0 off, 1 per stage, 2 + per conv launch */
/* The same switch WITHOUT discarding the records already taken (byolo_set_profiling invalidates them): a caller that times a
 * run of forwards records every n-th one (an event costs the GPU a few microseconds; ~95 per forward) and reads them all afterwards. */
BYOLO_API int32_t byolo_resume_profiling(byolo_t* h, int32_t on);
BYOLO_API int32_t byolo_stage_ms(byolo_t* h, float ms[4]);
/* Keep the records of the last `depth` profiled forwards (default 1) and choose which one byolo_stage_ms /
 * byolo_num_steps / byolo_step_profile / byolo_step_split read: age 0 = the last forward, 1 = the one before, ...
 * A caller timing K back-to-back forwards sets depth = K and reads every record after the run -- no host
 * synchronisation inside the timed region (bench.py). */
BYOLO_API int32_t byolo_set_profile_depth(byolo_t* h, int32_t depth);
BYOLO_API int32_t byolo_select_profile(byolo_t* h, int32_t age);
/* per kernel launch of the convolution stack in the LAST forward (profiling level 2): graph layer, kernel variant --
 *   128 / 64 / 32   conv_igemm_kernel, BN of the tile (split precision: + 1000 the general loop, + 2000 the 1x1 loop, + 3000 the
 *                   shared-tap 3x3 loop; 140 / -4 Winograd in split arithmetic: fused launch / input transform)
 *                                                                -1   the direct small-Cin kernels
 *   -2 / -3         Winograd input / output transform            129  the row-streaming Winograd-domain GEMM
 *   130             the same with output transform + epilogue    131 / 132  a 1x1 convolution / detection head as a
 *                   fused in (wino_fused_kernel)                            row-streaming launch, 128- / 64-wide tile
 * -- the EXECUTED extents {M, N, K} (for a Winograd-domain GEMM: 16 * tiles rows, cout, cin), the launch's device time
 * (hipEvents on `stream` around it) and the ALGORITHMIC FLOPs it stands for (2*M*N*K of the layer as written; differs
 * from the executed work for the T-invariant de-duplicated launches -- conv once per image + T masked epilogues; the
 * per-image partial sum of a concat's tiled half carries 0 -- and for Winograd, where the GEMM launch carries the
 * direct-convolution FLOPs of its samples and the transforms carry 0).
 * byolo_num_steps = launches of the last profiled forward. */
BYOLO_API int32_t byolo_num_steps(const byolo_t* h);
BYOLO_API int32_t byolo_step_profile(byolo_t* h, int32_t i, int32_t* layer, int32_t* variant, int64_t mnk[3], float* ms,
                                     double* algo_flops);
/* the same launch's split-K plan: K slices per tile of its last partial round of tiles (1 = not split) and how many
 * tiles were cut; a NEGATIVE ksplit -G = a stream-K launch: G workgroups share all tiles * K-tiles units evenly
 * (conv_igemm.hip; decided per (B, T) shape, deterministic).  A Winograd GEMM entry (variant 140): ksplit 1, split_tiles = the
 * output channels per workgroup the planner chose (256 | 128). */
BYOLO_API int32_t byolo_step_split(byolo_t* h, int32_t i, int32_t* ksplit, int32_t* split_tiles);
/* analytic cost of one forward: conv FLOPs (2*MAC, graph as written) for B images x T samples */
BYOLO_API int32_t byolo_flops(byolo_t* h, int32_t B, int32_t T, double* flops);

/* ---- input feed helper (host only): CRC-32C of the TFRecord framing read by the reference's
 * tf.data.TFRecordDataset (lib_yolo/dataset_utils.py:188-199); returns the raw (unmasked) CRC. */
BYOLO_API uint32_t byolo_crc32c(const void* h_data, size_t n);


/* ---- input feed, device side: `tf.image.convert_image_dtype(img, tf.float32)` of decode_img
 * (lib_yolo/dataset_utils.py:6-11) on the device -- d_f32[i] = float(d_u8[i]) * (1 / 255) in fp32, bit for bit the value the
 * host conversion produces -- so that the feed ships one byte per pixel-channel over PCIe instead of four.  n = elements
 * (B * H * W * C); d_f32 is what byolo_forward takes as d_img. */
BYOLO_API int32_t byolo_normalize_u8(byolo_t* h, const uint8_t* d_u8, int64_t n, float* d_f32, void* stream);

/* ---- training feed, device side (csrc/augment.hip): the crop and augmentation of lib_yolo/data_augmentation.py for one batch
 * in ONE launch (up to 32 images; larger batches are split into launches of 32).  Per image a plan (byolo/augment.py draws
 * them); per output pixel, in this order: u8 * (1 / 255) (as byolo_normalize_u8) -> crop window (y0, x0, ch, cw) -> TF1 legacy
 * bilinear resize to out_h x out_w when `rescale` (else ch == out_h and cw == out_w) -> left-right flip -> box blur k x k (SAME,
 * zero padding) -> colour op -> noise op (counter-based hash keyed by noise_key: the stream is documented in augment.hip).
 * Image b of d_u8 starts at byte b * img_stride and holds src_h rows of src_w * 3 bytes: the frame's rows row0 .. row0 + src_h - 1
 * (a caller may ship only the band of rows its crop reads; row0 = 0 for whole frames).  d_out: float32 [B, out_h, out_w, 3],
 * 4-byte aligned.  A plan out of range (window outside the shipped rows or the frame width, blur_k not in {0, 2, 3}, an unknown
 * op code, flip / rescale not 0 / 1, a parameter that is not finite, a hue delta outside [-1, 1]) is BYOLO_ERR_ARG before
 * anything is launched.  h may be NULL (errors: byolo_last_error(NULL)). */
enum { BYOLO_AUG_COLOR_NONE = 0, BYOLO_AUG_SATURATION = 1, BYOLO_AUG_BRIGHTNESS = 2, BYOLO_AUG_HUE = 3 };
enum { BYOLO_AUG_NOISE_NONE = 0, BYOLO_AUG_COLORED_SALT_N_PEPPER = 1, BYOLO_AUG_SALT_N_PEPPER = 2, BYOLO_AUG_GAUSSIAN = 3 };
typedef struct byolo_aug_plan {
    int32_t y0, x0, ch, cw;        /* crop window in frame coordinates                                                          */
    int32_t row0;                  /* first frame row shipped for this image (y0 >= row0, y0 - row0 + ch <= src_h)              */
    int32_t rescale, flip, blur_k; /* 0 / 1, 0 / 1, 0 | 2 | 3                                                                    */
    int32_t color_op, noise_op;    /* BYOLO_AUG_COLOR_* / BYOLO_AUG_NOISE_*                                                      */
    float color_param;             /* saturation factor, brightness delta or hue delta                                          */
    float noise_param;             /* salt-and-pepper amount or Gaussian stddev                                                 */
    uint64_t noise_key;            /* key of the per-element hash                                                               */
} byolo_aug_plan;
BYOLO_API int32_t byolo_augment_batch(byolo_t* h, const uint8_t* d_u8, int32_t B, int32_t src_h, int32_t src_w, int64_t img_stride,
                                      const byolo_aug_plan* h_plans, int32_t out_h, int32_t out_w, float* d_out, void* stream);

/* The two status words (byolo_status: {flags, layer}) copied device-to-device into d_out[2] on `stream`, without waiting: a
 * multi-GPU driver appends them to the buffer its ONE all-gather carries, so that every rank learns of any rank's
 * BYOLO_ERR_RANGE from the gathered list and all ranks switch to the fp32 mode together (byolo/inference.py). */
BYOLO_API int32_t byolo_copy_status(byolo_t* h, uint32_t* d_out, void* stream);

/* ---- input feed, host side: `tf.image.decode_png(encoded, dtype=tf.uint8)` of decode_img for the n records of a batch on
 * `threads` host threads -- the `map(parse_example, num_parallel_calls=config['cpu_thread_cnt'])` stage of TestingDataset
 * (lib_yolo/dataset_utils.py:196).  h_out: n frames of img_h * img_w * img_c bytes (e.g. pinned memory); status[i] per record:
 * OK, UNSUPPORTED (interlaced / palette / 16-bit: the caller decodes that record with a general decoder), SHAPE (the PNG is
 * not img_h x img_w x img_c; found_shape[3*i..] = what it is, like the reference's set_shape failure) or CORRUPT (signature,
 * chunk CRC, zlib stream, filter type).  Returns the number of records that are not OK, or BYOLO_ERR_ARG. */
enum { BYOLO_PNG_OK = 0, BYOLO_PNG_UNSUPPORTED = 1, BYOLO_PNG_SHAPE = 2, BYOLO_PNG_CORRUPT = 3 };
BYOLO_API int32_t byolo_png_decode_batch(const uint8_t* const* h_png, const size_t* png_bytes, int32_t n, int32_t img_h,
                                         int32_t img_w, int32_t img_c, uint8_t* h_out, int32_t threads, int32_t* status,
                                         int32_t* found_shape);

/* The whole map stage for the n records of a batch, natively: record i = lengths[i] payload bytes at offsets[i] of the open file
 * fds[i] (TFRecord framing: the payload is followed by its masked CRC-32C, checked if verify_crc) -> tf.train.Example -> the
 * first bytes value of `image/encoded` decoded as above into frame i of h_out, the first value of `image/filename` into
 * h_names[i * name_cap ...] (NUL-terminated UTF-8).  status[i] = BYOLO_PNG_* or BYOLO_FEED_IO (short read) / _CRC / _PROTO
 * (malformed Example, no image, a name of name_cap bytes or more).  Returns the number of records that are not OK. */
enum { BYOLO_FEED_IO = 4, BYOLO_FEED_CRC = 5, BYOLO_FEED_PROTO = 6 };
BYOLO_API int32_t byolo_feed_records(const int32_t* fds, const int64_t* offsets, const int64_t* lengths, int32_t n, int32_t verify_crc,
                                     int32_t img_h, int32_t img_w, int32_t img_c, uint8_t* h_out, int32_t threads, char* h_names,
                                     int32_t name_cap, int32_t* status, int32_t* found_shape);

/* ---- output writer, host side: the text `json.dump({'children': [bbox_to_ecp_format(b, ...) for b in boxes]}, f)` writes for
 * the kept rows of ONE image (inference_epistemic.py:84-92 + :131-170; inference_aleatoric.py:139-178;
 * inference_standard_yolov3.py:128-150), byte for byte: keys in the reference's order, coordinates scaled in float32 then
 * widened, score = obj * cls[argmax] in double, every number as CPython's float repr (shortest round-trip digits, NaN /
 * Infinity spelt as json.dump does), the index quirks of the reference kept (aleatoric: cls_entropy / layer_id / prior_id all
 * read column cls_start + C; epistemic: ped_score / rider_score = columns 17 / 18).  kind = BYOLO_DET_*; h_rows [n_rows,
 * row_len]; identity = labels[argmax + implicit_background] if that entry exists and is not NULL (ASCII without quotes /
 * backslashes), else the integer.  Returns the length of the text; if it exceeds cap nothing useful is in h_out and the
 * return value is -(length) - 16. */
BYOLO_API int64_t byolo_format_ecp_json(int32_t kind, const float* h_rows, int32_t n_rows, int32_t row_len, int32_t img_h,
                                        int32_t img_w, int32_t cls_cnt, int32_t obj_idx, int32_t cls_start,
                                        int32_t implicit_background, const char* const* labels, int32_t n_labels,
                                        char* h_out, size_t cap);

/* ---- head training with a frozen Darknet-53 (lib_yolo/train.py:53-54, :84-88 with 'freeze_darknet53': True, the only setting of
 * the reference's uncertainty_training.py:30, yolov3_training.py:29, pretraining.py:29; csrc/train_heads.hip).
 * A trainer is bound to a finalized handle whose graph has byolo_mark_backbone_end and, after it, stride-1 1x1 / 3x3 convolutions
 * with batch norm, routes, upsamplings and standard / aleatoric detection layers (no T stacking: the Bayesian model with
 * inference_mode=False).  byolo_trainer_create copies the head variables out of the handle: every convolution kernel, BN gamma /
 * beta, detection kernel / bias after the marker (its trainable variables, TF creation order), their gradients and Adam slots
 * (zero), and the heads' moving statistics.  It is host-only (the handle need not be finalized yet); the device copy is made by
 * the first call that needs it.  The library owns that state until byolo_trainer_destroy; errors are reported on the bound handle
 * (byolo_last_error(h)).  Lifetime: destroy the trainer BEFORE its handle and its fallback handle -- every call but
 * byolo_trainer_destroy reads them; byolo_trainer_set_fallback(tr, NULL) unbinds a fallback that is about to go.  aleatoric_loss: the flag of lib_yolo/layers.py:150-153 for every layer.
 *
 * byolo_trainer_step = one sess.run([train_step, ...]) on d_img [B,H,W,3] (device):
 *   backbone  byolo_forward's launches up to the marker on the bound handle, in its precision; if an activation leaves the split-f16
 *             range the step fails with BYOLO_ERR_RANGE before anything changed -- or, with a fallback handle set
 *             (byolo_trainer_set_fallback: an fp32 handle of the same graph and weights), runs the backbone there;
 *   heads     conv -> dropout (rate = cfg.drop_prob, inverted, where the layer has it) -> BN over the batch's B*H*W (biased
 *             variance, eps 1e-5) -> leaky 0.1; detection conv + bias.  Dropout keeps from byolo_rng.h keyed by (seed + step *
 *             0x9E3779B97F4A7C15, dropout ordinal), or d_mask_bits laid out as byolo_mask_layout(h, B, 1, ordinal) describes;
 *   loss      byolo_loss per detection layer on the ground truth of byolo_encode_gt (d_gt_* at prior box 0 of layer 0, N of all
 *             layers per image), L2 0.0005 * sum(w^2) / 2 over every kernel and detection bias of the HANDLE (the frozen ones
 *             are a constant); d_losses[6] (device doubles) = total, detection, regularization, loc, obj, cls (pre-update weights);
 *   backward  gradients of the total loss (L2 term included) with respect to every trainable variable, all in fp32;
 *   update    unless grads_only: moving mean / variance -= (moving - batch) * (1 - 0.99) with the BESSEL-CORRECTED batch variance
 *             (TF 1.x fused batch norm), then Adam (b1 0.9, b2 0.999, eps 1e-8, TF1's lr_t = lr sqrt(1 - b2^t) / (1 - b1^t),
 *             t = step + 1), and the step counter advances.
 * Everything is enqueued on `stream` (split precision: the step waits once, after the backbone, for the range status).  Results
 * are deterministic: two steps on the same inputs give the same bits.  d_workspace >= byolo_trainer_workspace_bytes(B); the
 * last step's activations stay readable in it (byolo_trainer_layer_output).
 * byolo_trainer_get / _set: host copies of a variable by TF name: slot 0 the value, 1 its gradient of the last step, 2 `<name>/Adam`,
 * 3 `<name>/Adam_1`; the heads' `.../moving_mean` / `.../moving_variance` in slot 0.  Both synchronise the device.
 * byolo_trainer_export: every trained variable and moving statistic into `dst` (byolo_set_param by name; dst is then un-finalized:
 * finalize it to run inference with them).
 * byolo_trainer_taps: the backbone layers the heads read (returns how many; fills up to cap indices).
 * byolo_trainer_layer_output: NHWC shape (d_dst NULL) or a device copy of a tap's or head convolution's output of the last step
 * (detection layers: the raw output, dense). */
typedef struct byolo_trainer byolo_trainer_t;
BYOLO_API int32_t byolo_trainer_create(byolo_t* h, int32_t aleatoric_loss, byolo_trainer_t** out);
BYOLO_API int32_t byolo_trainer_destroy(byolo_trainer_t* tr);
BYOLO_API int32_t byolo_trainer_set_fallback(byolo_trainer_t* tr, byolo_t* h_f32);
BYOLO_API int32_t byolo_trainer_workspace_bytes(byolo_trainer_t* tr, int32_t B, size_t* bytes);
BYOLO_API int32_t byolo_trainer_step(byolo_trainer_t* tr, const float* d_img, int32_t B, uint64_t seed, const uint32_t* d_mask_bits,
                                     const float* d_gt_loc, const float* d_gt_obj, const int32_t* d_gt_cls, const float* d_gt_ign,
                                     float lr, int32_t grads_only, double* d_losses, void* d_workspace, size_t workspace_bytes,
                                     void* stream);
BYOLO_API int32_t byolo_trainer_num_vars(const byolo_trainer_t* tr);
BYOLO_API int32_t byolo_trainer_var_info(const byolo_trainer_t* tr, int32_t i, const char** name, int32_t* ndim, int64_t shape[4]);
BYOLO_API int32_t byolo_trainer_get(byolo_trainer_t* tr, const char* name, int32_t slot, float* h_data, int64_t count);
BYOLO_API int32_t byolo_trainer_set(byolo_trainer_t* tr, const char* name, int32_t slot, const float* h_data, int64_t count);
BYOLO_API int32_t byolo_trainer_get_step(const byolo_trainer_t* tr, int64_t* step);
BYOLO_API int32_t byolo_trainer_set_step(byolo_trainer_t* tr, int64_t step);
BYOLO_API int32_t byolo_trainer_export(byolo_trainer_t* tr, byolo_t* dst);
BYOLO_API int32_t byolo_trainer_taps(const byolo_trainer_t* tr, int32_t* layers, int32_t cap);
BYOLO_API int32_t byolo_trainer_layer_output(byolo_trainer_t* tr, int32_t layer, float* d_dst, int64_t count, int64_t shape[4],
                                             void* stream);

/* ---- evaluation: detections against ground truth (no counterpart in the reference, whose ECP-JSON goes to an external
 * toolkit) ---------------------------------------------------------------------------------------------------------------
 * An evaluator is its own handle (no byolo_t): it scores the kept rows of byolo_sort_nms / byolo_forward (d_rows, d_count) on
 * labelled frames, one kernel launch per batch on the caller's stream, with no allocation and no host wait, and appends one
 * record per surviving detection to a CALLER-OWNED device table.  INTEGRATION.md ("Evaluation") has the definitions in full.
 *   class of a row   first index of the largest class score;  score = obj * cls[class], one float32 multiply; rows whose score
 *                    is NaN or below min_score are dropped
 *   ground truth     d_gt_boxes [B, gmax, 4] normalised (ymin, xmin, ymax, xmax), d_gt_labels [B, gmax] 0-based, d_gt_counts
 *                    [B]; a box whose label is outside [0, cls_cnt) is neither counted nor matchable
 *   matching         per image, rows in descending score (ties: lower row), each takes the not-yet-matched box of its class
 *                    with the largest IoU (ties: lower box index; the NMS's float32 IoU, a non-finite one counts as 0): a
 *                    true positive iff that IoU >= iou_thresh, and only then is the box marked
 *   record           record_words = BYOLO_EVAL_RECORD_HEAD + n_unc 32-bit words: int32 image sequence number (0 for the first
 *                    image after byolo_eval_reset), int32 row, int32 class, float score, int32 tp, int32 matched box or -1,
 *                    float best IoU (0 without an eligible box), then the row's columns unc_cols[0 .. n_unc) as floats.  The
 *                    records of an image are in matching order, images in the order they were added.
 * d_table holds `capacity` records, d_state byolo_eval_state_bytes(cls_cnt) bytes (running offset, per-class counts of eligible
 * boxes, image count, a sticky overflow word); both stay the caller's and must outlive the handle's use.  Records beyond the
 * capacity are dropped -- nothing is written outside the table -- and byolo_eval_finish then returns BYOLO_ERR_NOMEM (the
 * summary is filled all the same).  Limits: cap <= 4096 rows per image, gmax <= BYOLO_EVAL_MAX_GT.
 * byolo_eval_reset must run once before the first byolo_eval_add.  byolo_eval_finish and byolo_eval_records wait for `stream`. */
#define BYOLO_EVAL_MAX_GT 1024
#define BYOLO_EVAL_MAX_UNC 16
#define BYOLO_EVAL_RECORD_HEAD 7
typedef struct byolo_eval byolo_eval_t;
typedef struct byolo_eval_cfg {
    int32_t struct_bytes;          /* sizeof(byolo_eval_cfg) of the caller's header: a mismatch is BYOLO_ERR_ARG */
    int32_t row_len, obj_idx, cls_start_idx, cls_cnt;
    int32_t n_unc;
    int32_t unc_cols[BYOLO_EVAL_MAX_UNC];
    float iou_thresh, min_score;
} byolo_eval_cfg;
typedef struct byolo_eval_summary {
    int32_t struct_bytes;          /* set by the caller, as above */
    int32_t overflow;              /* the sticky word: detections were dropped */
    int32_t record_words;
    int32_t reserved;
    int64_t n_records;             /* records in the table: min(n_seen, capacity) */
    int64_t n_seen;                /* surviving detections of every image added */
    int64_t n_images;
} byolo_eval_summary;
BYOLO_API size_t byolo_eval_state_bytes(int32_t cls_cnt);
BYOLO_API int32_t byolo_eval_create(const byolo_eval_cfg* cfg, void* d_table, int64_t capacity, void* d_state, byolo_eval_t** out);
BYOLO_API int32_t byolo_eval_destroy(byolo_eval_t* ev);
BYOLO_API const char* byolo_eval_last_error(const byolo_eval_t* ev);
BYOLO_API int32_t byolo_eval_reset(byolo_eval_t* ev, void* stream);
BYOLO_API int32_t byolo_eval_add(byolo_eval_t* ev, const float* d_rows, int32_t B, int32_t cap, const int32_t* d_count,
                                 int64_t count_stride, const float* d_gt_boxes, const int32_t* d_gt_labels,
                                 const int32_t* d_gt_counts, int32_t gmax, void* stream);
BYOLO_API int32_t byolo_eval_finish(byolo_eval_t* ev, byolo_eval_summary* out, int64_t* h_class_gt, int32_t n_classes, void* stream);
BYOLO_API int32_t byolo_eval_records(byolo_eval_t* ev, int32_t* h_dst, int64_t first, int64_t n_records, void* stream);

/* Localisation residuals (aleatoric and Bayesian rows; INTEGRATION.md "Evaluation" has the definitions).  With a loc table set,
 * byolo_eval_add launches a second kernel right behind the matching on the same stream that writes, for every record of the
 * batch and at the record's index, BYOLO_EVAL_LOC_WORDS 32-bit words:
 *   0 .. 3  float residual r_x, r_y, r_w, r_h = t(matched ground-truth box) - t(detection): both boxes taken back to the raw
 *           location values at the detection's own cell and prior (the row's layer_col / prior_col columns name them), in
 *           float64, rounded once to float32
 *   4       int32 flags: bits 0 - 3 the coordinate's residual is valid, bit 4 tp, bit 5 the row's ids are valid, bits 8 - 15
 *           the layer, bits 16 - 23 the prior (both 0 with invalid ids)
 *   5       int32 cell iy * lw + ix
 * A record that is not a true positive, or whose ids are not finite, integral and inside this table, has residuals 0, valid
 * bits 0 and cell 0.  lh / lw: the layer's grid; prior_w / prior_h: the priors as the decode uses them (normalised).
 * d_loc_table holds byolo_eval_loc_bytes(capacity) bytes, caller-owned, 4-byte aligned; NULL switches the residuals off.
 * byolo_eval_set_loc is refused with BYOLO_ERR_STATE between the first byolo_eval_add and the next byolo_eval_reset, and with
 * BYOLO_ERR_ARG (message: the argument) otherwise.  The main records are the same bytes with and without it. */
#define BYOLO_EVAL_LOC_WORDS 6
#define BYOLO_EVAL_LOC_MAX_LAYERS 8
#define BYOLO_EVAL_LOC_MAX_PRIORS 16
typedef struct byolo_eval_loc_cfg {
    int32_t struct_bytes;          /* sizeof(byolo_eval_loc_cfg) of the caller's header: a mismatch is BYOLO_ERR_ARG */
    int32_t layer_col, prior_col, n_layers;
    int32_t lh[BYOLO_EVAL_LOC_MAX_LAYERS], lw[BYOLO_EVAL_LOC_MAX_LAYERS], n_priors[BYOLO_EVAL_LOC_MAX_LAYERS];
    float prior_w[BYOLO_EVAL_LOC_MAX_LAYERS][BYOLO_EVAL_LOC_MAX_PRIORS], prior_h[BYOLO_EVAL_LOC_MAX_LAYERS][BYOLO_EVAL_LOC_MAX_PRIORS];
} byolo_eval_loc_cfg;
BYOLO_API size_t byolo_eval_loc_bytes(int64_t capacity);
BYOLO_API int32_t byolo_eval_set_loc(byolo_eval_t* ev, const byolo_eval_loc_cfg* cfg, void* d_loc_table);
BYOLO_API int32_t byolo_eval_loc_records(byolo_eval_t* ev, int32_t* h_dst, int64_t first, int64_t n_records, void* stream);

/* The ladder: the matching at several IoU thresholds in one pass (AP50, AP75, AP averaged over 0.50 : 0.05 : 0.95;
 * INTEGRATION.md "Evaluation").  The matching DIFFERS per threshold -- a box that a detection fails to claim stays open for a
 * later one -- so the ladder is not derivable from the records of one threshold.  With a ladder table set, byolo_eval_add
 * launches one more kernel behind the matching on the same stream (no host wait) that matches every image of the batch once per
 * threshold, each threshold with its own matched set and otherwise by exactly the rule above (same survivors, same visiting
 * order, same float32 IoU, `iou >= thresholds[k]` compared in float32), and writes, for every record of the batch and at the
 * record's index, 1 + n_thr 32-bit words:
 *   0       int32 bit k is set iff the detection is a true positive at thresholds[k]
 *   1 + k   int32 the box it matched at thresholds[k], or -1
 * Thresholds need not be sorted or distinct.  d_ladder_table holds byolo_eval_ladder_bytes(capacity, n_thr) bytes, caller-owned,
 * 4-byte aligned; NULL switches the ladder off.  Nothing is written at or beyond `capacity` records.  byolo_eval_set_ladder is
 * refused with BYOLO_ERR_STATE between the first byolo_eval_add and the next byolo_eval_reset, and with BYOLO_ERR_ARG for a wrong
 * struct_bytes, n_thr outside 1 .. BYOLO_EVAL_LADDER_MAX, a threshold that is NaN or outside [0, 1] and a misaligned table.
 * The main records, the device state, the loc table and -- with no ladder set -- the launches are the same with and without it. */
#define BYOLO_EVAL_LADDER_MAX 16
typedef struct byolo_eval_ladder_cfg {
    int32_t struct_bytes;          /* sizeof(byolo_eval_ladder_cfg) of the caller's header: a mismatch is BYOLO_ERR_ARG */
    int32_t n_thr;
    float thresholds[BYOLO_EVAL_LADDER_MAX];
} byolo_eval_ladder_cfg;
BYOLO_API size_t byolo_eval_ladder_bytes(int64_t capacity, int32_t n_thr);
BYOLO_API int32_t byolo_eval_set_ladder(byolo_eval_t* ev, const byolo_eval_ladder_cfg* cfg, void* d_ladder_table);
BYOLO_API int32_t byolo_eval_ladder_records(byolo_eval_t* ev, int32_t* h_dst, int64_t first, int64_t n_records, void* stream);

/* The subsets: the matching per height range of the ground truth with ignore regions -- the protocol in which the pedestrian
 * benchmarks (EuroCity Persons, CityPersons, Caltech) publish LAMR; INTEGRATION.md "Evaluation" has the rule in full and
 * tests/_eval_subsets_ref.py restates it.  With a subsets table set, byolo_eval_add launches one more kernel behind the matching
 * on the same stream (no host wait) that matches every image of the batch once per subset s = [lo[s], hi[s]) of pixel heights
 * h = (ymax - ymin) * img_h (two float32 operations on the box as the matcher orders it):
 *   counted box    its label is a class and lo[s] <= h < hi[s]; only counted boxes can be matched, and only they are counted
 *   ignore region  for a detection of class c: every box whose label is outside [0, cls_cnt), every box of class c that is not
 *                  counted and, with ignore_other_classes, every box of another class.  Regions are never used up
 *   state          same survivors and visiting order as the main matching.  1: the counted, not yet matched box of the
 *                  detection's class with the largest IoU (ties: lower index) has IoU >= iou_thresh; the box is marked.
 *                  Else 2: the region with the largest inter / area(detection) (float32; 0 when either area is <= 0 or the
 *                  value is not finite; ties: lower index) reaches ignore_thresh.  Else 3: the detection's own height is
 *                  < lo[s] / height_slack or >= hi[s] * height_slack.  Else 0: a false positive.  States 2 and 3 are neither
 *                  true nor false positives
 *   record         at the record's index, 1 + n_subsets 32-bit words: word 0 holds the state of subset s at bits 2s, 2s + 1;
 *                  word 1 + s the matched box (state 1), the region (state 2), or -1
 *   counters       d_subsets_counts: n_subsets * cls_cnt int32, the counted boxes per (subset, class), subset-major
 * d_subsets_table holds byolo_eval_subsets_bytes(capacity, n_subsets) bytes and d_subsets_counts
 * byolo_eval_subsets_state_bytes(n_subsets, cls_cnt) bytes, both caller-owned and 4-byte aligned; byolo_eval_reset zeroes the
 * counters while they are set, so hand them over zeroed or reset afterwards.  A NULL table switches the subsets off.  Nothing
 * is written at or beyond `capacity` records.  byolo_eval_set_subsets is refused with BYOLO_ERR_STATE between the first
 * byolo_eval_add and the next byolo_eval_reset, and with BYOLO_ERR_ARG for a wrong struct_bytes, n_subsets outside
 * 1 .. BYOLO_EVAL_SUBSETS_MAX, a range that is NaN, negative or not lo < hi (hi may be +inf), img_h not finite and > 0,
 * ignore_thresh outside [0, 1], height_slack not finite and >= 1, NULL counters and a misaligned pointer.  The main records, the
 * device state, the other side tables and -- with no subsets set -- the launches are the same with and without it. */
#define BYOLO_EVAL_SUBSETS_MAX 16
typedef struct byolo_eval_subsets_cfg {
    int32_t struct_bytes;          /* sizeof(byolo_eval_subsets_cfg) of the caller's header: a mismatch is BYOLO_ERR_ARG */
    int32_t n_subsets;
    float lo[BYOLO_EVAL_SUBSETS_MAX];
    float hi[BYOLO_EVAL_SUBSETS_MAX];
    float img_h, ignore_thresh, height_slack;
    int32_t ignore_other_classes;
} byolo_eval_subsets_cfg;
BYOLO_API size_t byolo_eval_subsets_bytes(int64_t capacity, int32_t n_subsets);
BYOLO_API size_t byolo_eval_subsets_state_bytes(int32_t n_subsets, int32_t cls_cnt);
BYOLO_API int32_t byolo_eval_set_subsets(byolo_eval_t* ev, const byolo_eval_subsets_cfg* cfg, void* d_subsets_table, void* d_subsets_counts);
BYOLO_API int32_t byolo_eval_subsets_records(byolo_eval_t* ev, int32_t* h_dst, int64_t first, int64_t n_records, void* stream);
BYOLO_API int32_t byolo_eval_subsets_counts(byolo_eval_t* ev, int64_t* h_counts, int32_t n_counts, void* stream);

/* Probabilistic detection quality (Hall et al., WACV 2020; csrc/eval_pdq.hip; INTEGRATION.md "Evaluation" has the definition in
 * full, tests/_pdq_ref.py restates it).  With the PDQ tables set, byolo_eval_add launches three more kernels behind the matching
 * on the same stream (no host wait): the image's detections and counted boxes are listed, every (detection, box) pair gets its
 * spatial and label quality, and the one-to-one assignment that maximises the sum of pPDQ is found per image.  All float64.
 *   detections     kept rows whose score (class and score as above) is finite and >= cfg.min_score -- the evaluator's own
 *                  min_score is not applied --, in descending score, ties to the lower row.  More than BYOLO_PDQ_MAX_DET in one
 *                  image raise the overflow flag; none is dropped silently
 *   counted box    label inside [0, cls_cnt), finite corners and a non-empty pixel rectangle u in [ceil(X0 - 0.5), ceil(X1 - 0.5))
 *                  clipped to the frame (X0 = x0 * img_w ...).  No ignore handling
 *   detection      Gaussian corners: means X0 = x0 * img_w ..., sx^2 = max((var_cx + var_w / 4) * img_w^2, var_floor) with var_cx,
 *                  var_w as the variance voting forms them (var, ale_col, epi_col, geom as there; BYOLO_VOTE_NONE: 0).
 *                  px[u] = Phi((u + 0.5 - X0) / sx) * Phi((X1 - u - 0.5) / sx), p(u, v) = px[u] * py[v], segment {p >= p_min}.
 *                  A row with a non-finite box value, bad ids or a variance that is not finite and >= 0 matches nothing
 *   pair           without a shared pixel every value is 0; otherwise L_FG = -(1 / |G|) sum over G of log(max(p if p >= p_min
 *                  else 0, eps)), L_BG = -(1 / |G|) sum over segment \ G of log(max(1 - p, eps)), Q_S = exp(-(L_FG + L_BG)),
 *                  Q_L = obj * cls[label] (one float32 multiply, clamped to [0, 1], NaN: 0), pPDQ = sqrt(Q_S * Q_L)
 *   assignment     shortest augmenting paths with potentials on cost = -pPDQ; the smaller side is the rows (equal: the
 *                  detections), the column minimum of a step goes to the lowest column on ties.  A true positive is an
 *                  assigned pair with pPDQ > 0
 *   image record   BYOLO_PDQ_RECORD_BYTES bytes at index (image sequence number): int32 n_det, n_gt, n_tp, flags (bit 0: the
 *                  image had too many detections and none was evaluated); float64 sum of pPDQ, Q_S, Q_L, exp(-L_FG),
 *                  exp(-L_BG) over the true positives in ascending detection order
 *   pair record    one per true positive, appended through an atomic cursor (images in no fixed order): int32 image, row, box,
 *                  0; float64 pPDQ, Q_S, Q_L, L_FG, L_BG
 * d_image_table / d_pair_table hold image_capacity / pair_capacity records, d_state byolo_eval_pdq_state_bytes() bytes (zeroed by
 * byolo_eval_reset while set), d_workspace byolo_eval_pdq_workspace_bytes(B, cap, gmax) bytes for the batch that is added (0: an
 * argument outside byolo_eval_add's limits); all caller-owned and 8-byte aligned.  A NULL image table switches PDQ off.  Nothing is
 * written beyond either capacity; a record that does not fit raises the overflow flag.  byolo_eval_add returns BYOLO_ERR_NOMEM,
 * before anything is launched, for a batch the workspace is too small for.
 * The workspace is the scratch of ONE byolo_eval_add and carries nothing to the next, so it alone may be replaced at any time,
 * also between two adds: byolo_eval_set_pdq_workspace(ev, d_workspace, workspace_bytes) -- a batch with more boxes per image than
 * any before it (gmax is a batch's own padding) needs a larger one.  The launches already on the stream keep the old pointer: free
 * it in stream order.  BYOLO_ERR_STATE without PDQ tables, BYOLO_ERR_ARG for a NULL or misaligned pointer.
 * byolo_eval_set_pdq is refused with BYOLO_ERR_STATE between the first byolo_eval_add and the next byolo_eval_reset, and with
 * BYOLO_ERR_ARG for a wrong struct_bytes, an unknown var or one whose columns the rows do not have, min_score NaN, p_min outside
 * (0, 1), eps outside (0, p_min], var_floor not finite and > 0, img_h / img_w outside 1 .. BYOLO_PDQ_MAX_FRAME, a geometry table
 * beyond its limits (geom may be NULL with BYOLO_VOTE_NONE), a capacity below 1, a NULL or misaligned pointer.
 * byolo_eval_pdq_images / _pairs wait for `stream`, store the number of records so far in *n_total (images: those added; pairs:
 * the cursor, which may exceed the capacity) and copy n_records records from `first`; BYOLO_ERR_NOMEM after the copy when the
 * overflow flag is up.
 * byolo_eval_pdq_matrix (for tests and tools; waits for `stream`): what the workspace holds of image `image` of the LAST
 * byolo_eval_add (B, cap, gmax its arguments, nd = min(cap, BYOLO_PDQ_MAX_DET)): h_counts [2] = n_det, n_gt (counted); h_rows [nd]
 * the detections' rows in matching order; h_gts [gmax] the counted boxes' indices; h_planes [5][nd][gmax] float64: pPDQ, Q_S, Q_L,
 * L_FG, L_BG of detection d and counted box c at [k][d][c].  Only the first n_det / n_gt entries of each are defined.
 * BYOLO_ERR_STATE before the first add behind byolo_eval_set_pdq or byolo_eval_set_pdq_workspace.
 * byolo_pdq_assign: the assignment stage alone on a float64 matrix [n_det, n_gt] of pPDQ on the device (row-major, both sides
 * 0 .. BYOLO_PDQ_MAX_DET, every entry finite); d_out_match [n_det] int32 receives each detection's box or -1. */
#define BYOLO_PDQ_MAX_DET 1024
#define BYOLO_PDQ_MAX_FRAME 4096
#define BYOLO_PDQ_RECORD_BYTES 56
typedef struct byolo_eval_pdq_cfg {
    int32_t struct_bytes;          /* sizeof(byolo_eval_pdq_cfg) of the caller's header: a mismatch is BYOLO_ERR_ARG */
    int32_t var;                   /* BYOLO_VOTE_* */
    int32_t ale_col, epi_col;      /* as in byolo_vote_cfg */
    int32_t img_h, img_w;
    float min_score;
    int32_t reserved;
    double p_min, eps, var_floor;
} byolo_eval_pdq_cfg;
BYOLO_API size_t byolo_eval_pdq_workspace_bytes(int32_t B, int32_t cap, int32_t gmax);
BYOLO_API size_t byolo_eval_pdq_state_bytes(void);
BYOLO_API int32_t byolo_eval_set_pdq(byolo_eval_t* ev, const byolo_eval_pdq_cfg* cfg, const byolo_eval_loc_cfg* geom, void* d_image_table,
                                     int64_t image_capacity, void* d_pair_table, int64_t pair_capacity, void* d_state, void* d_workspace,
                                     size_t workspace_bytes);
BYOLO_API int32_t byolo_eval_set_pdq_workspace(byolo_eval_t* ev, void* d_workspace, size_t workspace_bytes);
BYOLO_API int32_t byolo_eval_pdq_images(byolo_eval_t* ev, void* h_dst, int64_t first, int64_t n_records, int64_t* n_total, void* stream);
BYOLO_API int32_t byolo_eval_pdq_pairs(byolo_eval_t* ev, void* h_dst, int64_t first, int64_t n_records, int64_t* n_total, void* stream);
BYOLO_API int32_t byolo_eval_pdq_matrix(byolo_eval_t* ev, int32_t image, int32_t* h_counts, int32_t* h_rows, int32_t* h_gts, double* h_planes,
                                        void* stream);
BYOLO_API int32_t byolo_pdq_assign(const double* d_matrix, int32_t n_det, int32_t n_gt, int32_t* d_out_match, void* stream);

/* ---- variance voting (He et al., CVPR 2019; no counterpart in the reference; csrc/box_vote.hip; INTEGRATION.md "Variance voting"
 * has the definition in full, tests/_box_vote_ref.py restates it) -------------------------------------------------------------
 * After the NMS every kept row's box is replaced by the weighted mean of the pre-NMS boxes of its class that overlap it:
 *   voters of kept row k   rows i of the same image and the same class as the NMS decided it (agnostic: every NMS candidate is
 *                          class 0; otherwise the strict unique maximum of the class scores) with score >= min_score, the NMS's
 *                          float32 IoU(k, i) > iou_min, four finite box values and -- unless var == BYOLO_VOTE_NONE -- layer / prior
 *                          ids that are finite, integral and inside the geometry table, and variances that are finite and >= 0
 *   weights                p = exp(-(1 - iou)^2 / sigma_t), g_c = p / max(var_c, var_floor) per coordinate c of (cx, cy, w, h);
 *                          var_c = the row's variance of the raw location value, taken to box units at the row's own cell:
 *                          var_cx = v_x (fx (1 - fx) / lw)^2 with fx the centre's position inside its cell, var_w = v_w w^2
 *                          (BYOLO_VOTE_NONE: g_c = p); all float64 on the float32 inputs
 *   result                 c' = sum g_c c / sum g_c; columns 0 - 3 of the row become (cy' - h'/2, cx' - w'/2, cy' + h'/2, cx' + w'/2),
 *                          rounded once to float32; d_vote_n [B, cap] int32 receives the number of voters (0 in the padding)
 * Every other column and the padding rows are copied unchanged; d_kept / d_count are only read.  A kept row that is not among
 * its own voters keeps its bits and gets vote_n 0.  The sums are taken in a fixed order (fixed lane assignment, fixed reduction
 * tree): the result is deterministic and does not depend on the image's position in the batch.
 * sigma_t and var_floor have starting values (0.02, 1e-8) that nobody has tuned on a real checkpoint.
 * ale_col / epi_col: first of the four columns (x, y, w, h) of the aleatoric / epistemic variances in a row, -1 = the rows have
 * none (aleatoric rows: 4 / -1, Bayesian rows: 8 / 4); BYOLO_VOTE_TOTAL adds the two in float64.
 * byolo_box_vote: the stand-alone stage behind byolo_sort_nms (also: behind byolo_finish_tshard + byolo_sort_nms) on the same
 * d_boxes / nms_mode / obj_idx / cls_start_idx (BYOLO_NMS_PER_CLASS: the handle's cls_cnt).  geom: lh / lw / n_priors and the id
 * columns of byolo_eval_loc_cfg (the priors themselves are not read); NULL with BYOLO_VOTE_NONE.  d_rows_out may alias d_rows_in.
 * d_ws >= byolo_box_vote_workspace_bytes(B, N) (0 for B < 1 or N < 1), 8-byte aligned.  Refused with BYOLO_ERR_ARG before anything is
 * launched, the argument named in byolo_last_error: a wrong struct_bytes, sigma_t <= 0, iou_min < 0, var_floor <= 0 (or any of
 * them NaN), an unknown var, a var whose columns are -1, columns outside the row, a geometry table beyond its limits; a
 * workspace that is too small is BYOLO_ERR_NOMEM.
 * byolo_set_box_vote(h, cfg): byolo_forward votes in place on d_rows right behind the NMS (cfg NULL: off, the default; with it
 * off every output is what it was without this entry point).  ale_col / epi_col of cfg are ignored: the handle knows its rows
 * (standard rows take BYOLO_VOTE_NONE only, aleatoric rows not BYOLO_VOTE_EPI / _TOTAL), and the geometry is that of its detection
 * layers.  The stage's workspace is part of byolo_workspace_bytes while voting is on.  byolo_box_vote_counts: vote_n [B, cap] of
 * the handle's LAST byolo_forward with d_rows, copied to d_vote_n on `stream`; BYOLO_ERR_STATE without one. */
enum { BYOLO_VOTE_NONE = 0, BYOLO_VOTE_ALE = 1, BYOLO_VOTE_EPI = 2, BYOLO_VOTE_TOTAL = 3 };
typedef struct byolo_vote_cfg {
    int32_t struct_bytes;          /* sizeof(byolo_vote_cfg) of the caller's header: a mismatch is BYOLO_ERR_ARG */
    int32_t var;                   /* BYOLO_VOTE_* */
    float sigma_t, iou_min, min_score, var_floor;
    int32_t ale_col, epi_col;
} byolo_vote_cfg;
BYOLO_API size_t byolo_box_vote_workspace_bytes(int32_t B, int64_t N);
BYOLO_API int32_t byolo_box_vote(byolo_t* h, const float* d_boxes, int32_t B, int64_t N, int32_t D, int32_t obj_idx,
                                 int32_t cls_start_idx, int32_t nms_mode, const byolo_vote_cfg* cfg, const byolo_eval_loc_cfg* geom,
                                 const float* d_rows_in, const int32_t* d_kept, const int32_t* d_count, int32_t cap,
                                 float* d_rows_out, int32_t* d_vote_n, void* d_ws, size_t ws_bytes, void* stream);
BYOLO_API int32_t byolo_set_box_vote(byolo_t* h, const byolo_vote_cfg* cfg);
BYOLO_API int32_t byolo_box_vote_counts(byolo_t* h, int32_t* d_vote_n, int32_t B, int32_t cap, void* stream);

/* ---- soft-NMS (Bodla, Singh, Chellappa, Davis, ICCV 2017, Algorithm 1; no counterpart in the reference; csrc/tail_kernels.hip
 * soft_*; INTEGRATION.md "Soft-NMS" has the definition in full, tests/_soft_nms_ref.py restates it) ---------------------------
 * In place of the hard greedy NMS: per (image, class) -- the classes of byolo_sort_nms for the same nms_mode -- the candidate with
 * the largest CURRENT score is picked (ties: lower row index), and the current score of every remaining candidate i is multiplied
 * by a weight of v = the NMS's float32 IoU(pick, i):
 *   BYOLO_SOFT_NMS_LINEAR     w = 1 - v where v > iou_soft, else 1
 *   BYOLO_SOFT_NMS_GAUSSIAN   w = float32(exp(-(v * v) / sigma)), formed in float64
 * Candidates are the class's members with score > min_score; a candidate leaves when v > iou_hard (1: never) or its score is no
 * longer > min_score.  The walk ends after max_out picks or when no candidate is left.
 * Outputs as byolo_sort_nms (d_rows [B, cap, D] in pick order, class 0's first; d_kept; d_count; byolo_nms_class_counts), except
 * that column obj_idx of a kept row holds its score at the moment it was picked; within a class these are non-increasing.
 * Up to BYOLO_SOFT_NMS_RESIDENT candidates of one (image, class) are held in registers; beyond that (and for every class under
 * byolo_plan_opts.nms_general) a slower path keeps the current scores in the workspace -- same bytes.  Deterministic.
 * The defaults (Gaussian, sigma 0.5, iou_soft 0.3, iou_hard 1, min_score 0.001) are the paper's; nobody has tuned them on this
 * detector.  Refused with BYOLO_ERR_ARG, the field named in byolo_last_error: a wrong struct_bytes, an unknown method, sigma not
 * > 0 and finite, iou_soft / iou_hard outside [0, 1], min_score negative or not finite.
 * d_ws >= byolo_soft_nms_workspace_bytes(B, N, nms_mode, cls_cnt) (0 for arguments the mode refuses).
 * byolo_set_soft_nms(h, cfg): byolo_forward runs this stage in place of the hard NMS (cfg NULL: off, the default; with it off every
 * output is what it was without this entry point); box voting (byolo_set_box_vote) then votes behind it.  Its workspace is part
 * of byolo_workspace_bytes while it is on. */
#define BYOLO_SOFT_NMS_RESIDENT 8192
enum { BYOLO_SOFT_NMS_LINEAR = 0, BYOLO_SOFT_NMS_GAUSSIAN = 1 };
typedef struct byolo_soft_nms_cfg {
    int32_t struct_bytes;          /* sizeof(byolo_soft_nms_cfg) of the caller's header: a mismatch is BYOLO_ERR_ARG */
    int32_t method;                /* BYOLO_SOFT_NMS_* */
    float sigma, iou_soft, iou_hard, min_score;
} byolo_soft_nms_cfg;
BYOLO_API size_t byolo_soft_nms_workspace_bytes(int32_t B, int64_t N, int32_t nms_mode, int32_t cls_cnt);
BYOLO_API int32_t byolo_soft_nms(byolo_t* h, const float* d_boxes, int32_t B, int64_t N, int32_t D, int32_t obj_idx,
                                 int32_t cls_start_idx, int32_t nms_mode, int32_t max_out, const byolo_soft_nms_cfg* cfg,
                                 void* d_ws, size_t ws_bytes, float* d_rows, int32_t* d_kept, int32_t* d_count, void* stream);
BYOLO_API int32_t byolo_set_soft_nms(byolo_t* h, const byolo_soft_nms_cfg* cfg);

/* ---- variance recalibration (sigma-scaling, Laves et al. 2020; no counterpart in the reference; csrc/var_recal.hip; INTEGRATION.md
 * "Variance recalibration" has the definitions in full, tests/_var_recal_ref.py restates them) -----------------------------------
 * A calibration is a table of float64 pairs (a, b) per detection layer l, prior p and coordinate c of (x, y, w, h); the calibrated
 * variance of a row is v' = a v^b, v the row's TARGET variance of that coordinate: BYOLO_VAR_RECAL_ALE the aleatoric column,
 * _EPI the epistemic column, _TOTAL their float64 sum -- ONE factor f = v' / v then multiplies both columns.
 * Apply (one thread per row of D floats; kind = BYOLO_DET_ALEATORIC rows of 14 + C or BYOLO_DET_EPISTEMIC rows of 21 + C columns):
 *   row       layer / prior from the last two columns; an id that is not finite, not integral or outside the table leaves the
 *             whole row untouched
 *   factor    b == 1 exactly: f = a.  Otherwise f = a exp((b - 1) log v), float64, and the coordinate is untouched unless v is
 *             finite and > 0
 *   column    float32(float64(col) f), rounded once; a NaN keeps its bits
 *   derived   aleatoric rows: column 8 = ((c4 c5) c6) c7; Bayesian rows: column 13 = (((0 + a0) + a1) + a2) + a3, both float32
 *             as the decode forms them, and column 12 = float32(float64(col12) P), P = ((fx fy) fw) fh over the epistemic
 *             factors (1 for an untouched coordinate; the column is left alone under _ALE and when it is NaN)
 * Every other column keeps its bits: the identity table (a = b = 1) reproduces its input.
 * byolo_var_recal_apply: the stand-alone stage, handle-less (errors: byolo_last_error(NULL)); d_out [n, D] must not overlap d_in;
 * d_table: BYOLO_VAR_RECAL_TABLE_BYTES bytes of device memory, 8-byte aligned, holding what byolo_var_recal_table(cfg, h_table)
 * wrote to the host buffer h_table of that size -- the caller copies it to the device ONCE per table, complete or ordered in front
 * of `stream`, and may use it for any number of calls: the call itself copies nothing and never waits.  Refused with BYOLO_ERR_ARG, the field named: a wrong struct_bytes, an unknown kind / target, a
 * target the rows do not have, D < 14 (aleatoric) or < 21 (Bayesian), n_layers / n_priors beyond the limits of byolo_eval_loc_cfg,
 * an a that is not finite and > 0, a b that is not finite.
 * byolo_set_var_recal(h, cfg): byolo_forward applies the table in place on the pre-NMS rows right behind the decode, so d_boxes,
 * d_rows, the soft-NMS and box voting see calibrated variances; the NMS reads no variance column, so d_kept / d_count do not
 * change (cfg NULL: off, the default; with it off every output is what it was without this entry point).  The handle keeps a
 * device copy of the table: no allocation and no host wait per forward.  kind and the geometry must be the handle's
 * (BYOLO_ERR_ARG names the field; BYOLO_ERR_STATE before the detection layers exist).  A T-shard forward hands out sums and
 * applies nothing: call byolo_var_recal_apply behind byolo_finish_tshard.
 * Fit (byolo_var_recal_fit): d_r / d_v [n] float64, the residuals and target variances of the eligible entries, grouped into
 * n_seg consecutive segments d_seg[s] .. d_seg[s + 1] (int64, n_seg + 1 offsets); one workgroup per segment, the whole Newton
 * iteration of BYOLO_VAR_RECAL_POWER inside the one launch.  Every sum is the FIXED SUM: partial[t] = the sequential sum of the
 * terms j = t (mod 256) in ascending j, the result the sequential sum of partial[0 .. 255]; float64, no atomics, the same bytes
 * in every run.  d_out [n_seg][BYOLO_VAR_RECAL_FIT_WORDS] float64: n, a, b, mean r^2 / v, NLL before, NLL after, iterations,
 * status (BYOLO_VAR_RECAL_FITTED, _SCALE_FALLBACK: power with n < 3, a singular Hessian or a step that is not finite -- the scale
 * answer with b = 1, _IDENTITY: sum r^2 / v is 0 or not finite, _EMPTY), converged, max |log v - mean log v|.
 * d_ws >= byolo_var_recal_fit_workspace_bytes(n), 8-byte aligned.  INTEGRATION.md has the Newton rule. */
#define BYOLO_VAR_RECAL_TABLE_BYTES 8192
#define BYOLO_VAR_RECAL_FIT_WORDS 10
enum { BYOLO_VAR_RECAL_ALE = 1, BYOLO_VAR_RECAL_EPI = 2, BYOLO_VAR_RECAL_TOTAL = 3 };
enum { BYOLO_VAR_RECAL_SCALE = 0, BYOLO_VAR_RECAL_POWER = 1 };
enum { BYOLO_VAR_RECAL_FITTED = 0, BYOLO_VAR_RECAL_SCALE_FALLBACK = 1, BYOLO_VAR_RECAL_IDENTITY = 2, BYOLO_VAR_RECAL_EMPTY = 3 };
typedef struct byolo_var_recal_cfg {
    int32_t struct_bytes;          /* sizeof(byolo_var_recal_cfg) of the caller's header: a mismatch is BYOLO_ERR_ARG */
    int32_t kind;                  /* BYOLO_DET_ALEATORIC or BYOLO_DET_EPISTEMIC: the layout of the rows */
    int32_t target;                /* BYOLO_VAR_RECAL_ALE / _EPI / _TOTAL */
    int32_t n_layers;
    int32_t n_priors[BYOLO_EVAL_LOC_MAX_LAYERS];
    double a[BYOLO_EVAL_LOC_MAX_LAYERS][BYOLO_EVAL_LOC_MAX_PRIORS][4];
    double b[BYOLO_EVAL_LOC_MAX_LAYERS][BYOLO_EVAL_LOC_MAX_PRIORS][4];
} byolo_var_recal_cfg;
BYOLO_API int32_t byolo_var_recal_table(const byolo_var_recal_cfg* cfg, double* h_table);
BYOLO_API int32_t byolo_var_recal_apply(const byolo_var_recal_cfg* cfg, const float* d_in, int64_t n, int32_t D, float* d_out,
                                        const void* d_table, void* stream);
BYOLO_API int32_t byolo_set_var_recal(byolo_t* h, const byolo_var_recal_cfg* cfg);
BYOLO_API size_t byolo_var_recal_fit_workspace_bytes(int64_t n);
BYOLO_API int32_t byolo_var_recal_fit(const double* d_r, const double* d_v, const int64_t* d_seg, int32_t n_seg, int64_t n,
                                      int32_t method, double* d_out, void* d_ws, size_t ws_bytes, void* stream);

/* ---- score recalibration (logistic map: Platt 1999, Guo et al. 2017; box-dependent covariates: Kueppers et al. 2020; no counterpart
 * in the reference; csrc/score_recal.hip; INTEGRATION.md "Score recalibration" has the definitions in full,
 * tests/_score_recal_ref.py restates them) ------------------------------------------------------------------------------------------
 * A calibration is a table w[g][k] of float64 weights over K features (2 <= K <= BYOLO_SCORE_RECAL_MAX_K) per group g: ONE group
 * (by = BYOLO_SCORE_RECAL_BY_ALL) or one per class (_BY_CLASS, cls_cnt <= BYOLO_SCORE_RECAL_MAX_GROUPS).  The calibrated score of a
 * kept row is s' = 1 / (1 + exp(-(w[g] . x))), float64, the dot product in ascending k.
 *   class, s   the first index of the largest class score (a NaN wins); s = obj * cls[class], one float32 multiply -- the
 *              evaluation's rule.  kind says where obj and the classes are (standard 4 / 5, aleatoric 9 / 11, Bayesian 14 / 17).
 *   features   feat_kind[0] is _F_BIAS (1), feat_kind[1] is _F_LOGIT: log(t / (1 - t)), t = min(max(s, 1e-7), 1 - 1e-7).
 *              _F_LOG_HEIGHT: log(h), h = col 2 - col 0 in float32, widened; 1e-6 where h is not finite or not > 1e-6.
 *              _F_COL_ID: the row's column feat_col[k]; 0 where it is not finite.  _F_COL_LOG: log(u) of that column; u = 1e-12
 *              where it is not finite or not > 1e-12.
 *   writes     score = float32(s'), and obj = float32(float64(score) / float64(cls[class])) so that obj * cls[class] downstream is
 *              the calibrated score within one float32 rounding.  The row is left alone and score = s where s is NaN, where
 *              cls[class] is not finite and > 0, and where the group's weights are the IDENTITY (0, 1, 0, ...): no exp, no log.
 * Every other column keeps its bits.  score [B, cap] is 0 in the padding (k >= count).
 * byolo_score_recal_apply: the stand-alone stage, handle-less (errors: byolo_last_error(NULL)) on kept rows d_rows_in [B, cap, D]
 * and d_count [B, 2] (the first word of each pair counts the kept rows, as byolo_forward writes it); d_rows_out must not overlap
 * d_rows_in; d_table: BYOLO_SCORE_RECAL_TABLE_BYTES bytes of device memory, 8-byte aligned, holding what byolo_score_recal_table
 * wrote to a host buffer of that size, copied to the device by the caller ONCE per table.  Refused with BYOLO_ERR_ARG, the field
 * named: a wrong struct_bytes, an unknown kind / by, cls_cnt outside the groups, K outside 2 .. 8, feat_kind[0] / [1] not bias /
 * logit, a feature column outside the row, D != the kind's row length, a weight that is not finite.
 * byolo_set_score_recal(h, cfg): byolo_forward applies the table in place on d_rows behind the NMS or soft-NMS and in front of box
 * voting, reading d_count on the device (cfg NULL: off, the default; with it off every output is what it was without this entry
 * point).  byolo_score_recal_scores then copies score [B, cap] of the last such forward, on `stream`.  A T-shard forward runs
 * no NMS: call byolo_score_recal_apply behind the caller's own.
 * byolo_score_recal_features: d_x [n, K] float64 of cfg's features from n float32 rows d_src of `stride` floats whose score is
 * the column score_col (records of an evaluation rather than kept rows); cols [K] on the host: the column of d_src of every
 * _F_COL_* feature; ymin_col / ymax_col: the two of _F_LOG_HEIGHT.
 * Fit (byolo_score_recal_fit): d_x [n, K] and d_y [n] (float64, 0 / 1), grouped into n_seg consecutive segments d_seg[s] ..
 * d_seg[s + 1]; one workgroup per segment standardises the features (population mean and standard deviation; a feature whose
 * standard deviation is 0 or not finite is dropped: weight 0), runs Newton on the ridge-penalised mean NLL (l2 >= 0, not on the
 * bias; Cholesky; the step halved at most 30 times while the loss does not fall; at most 50 iterations; converged at a step below
 * 1e-10) and folds the weights back, inside the one launch.  Every sum is the FIXED SUM of byolo_var_recal_fit.  d_out
 * [n_seg][BYOLO_SCORE_RECAL_FIT_WORDS] float64: n, positives, status (_FIT; _IDENTITY: n < min_n, no positive or no negative;
 * _EMPTY), iterations, converged, NLL before, NLL after, Brier before, Brier after, the last step, the dropped features as a bit
 * mask, one spare word, then w[8], mean[8], sd[8].  d_ws >= byolo_score_recal_fit_workspace_bytes(n, K), 8-byte aligned. */
#define BYOLO_SCORE_RECAL_MAX_K 8
#define BYOLO_SCORE_RECAL_MAX_GROUPS 80
#define BYOLO_SCORE_RECAL_TABLE_BYTES 5120
#define BYOLO_SCORE_RECAL_FIT_WORDS 36
enum { BYOLO_SCORE_RECAL_BY_ALL = 0, BYOLO_SCORE_RECAL_BY_CLASS = 1 };
enum { BYOLO_SCORE_RECAL_F_BIAS = 0, BYOLO_SCORE_RECAL_F_LOGIT = 1, BYOLO_SCORE_RECAL_F_LOG_HEIGHT = 2, BYOLO_SCORE_RECAL_F_COL_ID = 3,
       BYOLO_SCORE_RECAL_F_COL_LOG = 4 };
enum { BYOLO_SCORE_RECAL_FIT = 0, BYOLO_SCORE_RECAL_IDENTITY = 1, BYOLO_SCORE_RECAL_EMPTY = 2 };
typedef struct byolo_score_recal_cfg {
    int32_t struct_bytes;          /* sizeof(byolo_score_recal_cfg) of the caller's header: a mismatch is BYOLO_ERR_ARG */
    int32_t kind;                  /* BYOLO_DET_STANDARD / _ALEATORIC / _EPISTEMIC: the layout of the rows */
    int32_t cls_cnt;
    int32_t by;                    /* BYOLO_SCORE_RECAL_BY_ALL / _BY_CLASS */
    int32_t K;
    int32_t feat_kind[BYOLO_SCORE_RECAL_MAX_K];   /* BYOLO_SCORE_RECAL_F_* */
    int32_t feat_col[BYOLO_SCORE_RECAL_MAX_K];    /* the row's column of a _F_COL_* feature */
    int32_t reserved;
    double w[BYOLO_SCORE_RECAL_MAX_GROUPS][BYOLO_SCORE_RECAL_MAX_K];
} byolo_score_recal_cfg;
BYOLO_API int32_t byolo_score_recal_table(const byolo_score_recal_cfg* cfg, double* h_table);
BYOLO_API int32_t byolo_score_recal_apply(const byolo_score_recal_cfg* cfg, const float* d_rows_in, const int32_t* d_count, int32_t B,
                                          int32_t cap, int32_t D, float* d_rows_out, float* d_score, const void* d_table, void* stream);
BYOLO_API int32_t byolo_set_score_recal(byolo_t* h, const byolo_score_recal_cfg* cfg);
BYOLO_API int32_t byolo_score_recal_scores(byolo_t* h, float* d_score, int32_t B, int32_t cap, void* stream);
BYOLO_API int32_t byolo_score_recal_features(const byolo_score_recal_cfg* cfg, const float* d_src, int64_t n, int32_t stride,
                                             int32_t score_col, int32_t ymin_col, int32_t ymax_col, const int32_t* cols, double* d_x,
                                             void* stream);
BYOLO_API size_t byolo_score_recal_fit_workspace_bytes(int64_t n, int32_t K);
BYOLO_API int32_t byolo_score_recal_fit(const double* d_x, const double* d_y, const int64_t* d_seg, int32_t n_seg, int64_t n,
                                        int32_t K, double l2, int64_t min_n, double* d_out, void* d_ws, size_t ws_bytes, void* stream);

/* ---- test-time augmentation (mirrored and rescaled views merged in front of the NMS; no counterpart in the reference;
 * csrc/tta.hip; INTEGRATION.md "Test-time augmentation" has the definitions in full, tests/_tta_ref.py restates them) ----------
 * A view is the same frame mirrored left-right and / or at a second size.  Every view's pre-NMS rows go into ONE candidate set
 * per image, the union [B, Nu, D] with Nu = sum Nv and the views in order; byolo_sort_nms / byolo_soft_nms, byolo_box_vote and
 * byolo_score_recal_apply then run on the union as on any rows.  byolo_forward is not involved: byolo/tta.py composes the stages.
 * byolo_tta_view_f32: float32 frames d_in [B, src_h, src_w, 3] -> d_out [B, out_h, out_w, 3]: TF1's legacy bilinear resize
 * (src = dst * in / out, no half-pixel offset; skipped when the sizes are equal) and the left-right flip of byolo_augment_batch,
 * operation for operation: the bytes byolo_augment_batch writes for the whole uint8 frame whose * (1.0f / 255.0f) is d_in.  The same
 * size with flip is a mirrored copy.  Handle-less (errors: byolo_last_error(NULL)); d_out must not overlap d_in; B < 1 is a no-op.
 * byolo_tta_merge: one view's rows d_rows [B, Nv, D] -> rows row_off .. row_off + Nv - 1 of d_union [B, Nu, D]; the other rows of
 * the union are not touched.  Boxes are normalised: a rescaled view needs no coordinate change.  flip: column 1 = 1.0f - column 3
 * and column 3 = 1.0f - column 1 (one float32 rounding; a NaN keeps its bits); the variances of the raw location values and the
 * 4 x 4 determinant do not change under t_x -> -t_x.  size_idx g (the view's size among the distinct sizes, 0 = the model's own):
 * column layer_col gains 3 g as a float (exact; g = 0 and a non-finite id keep their bits), so that the ids of all views index ONE
 * byolo_eval_loc_cfg of 3 n_sizes layers -- the geometry byolo_box_vote, the localisation residuals and the PDQ take for merged
 * rows.  kind: BYOLO_DET_*, D = 5 + C / 14 + C / 21 + C with C in 1 .. 128; layer_col: -1 for standard rows (they have no ids),
 * D - 2 otherwise.  Handle-less.  Refused with BYOLO_ERR_ARG, the argument named, before anything is launched: a D the kind cannot
 * have, a layer_col that is not the kind's, row_off + Nv beyond Nu, a NULL or misaligned pointer, a union that overlaps the rows.
 * B < 1 or Nv < 1 is a no-op.
 * byolo_tta_support: behind the NMS on the union (d_kept / d_count of byolo_sort_nms or byolo_soft_nms on d_union with the same
 * obj_idx / cls_start_idx / nms_mode).  The kept row k is the union row d_kept[b][k] (its box before any voting).  For every kept
 * row of the d_count[b][0] real ones and every view v, the WITNESS is the union row i in view_off[v] .. view_off[v + 1] - 1 of the
 * same image with: the class of k as the NMS decides it (a row of no class has no witness and is none); score >= min_score; four
 * finite box values; IoU(k, i) > iou_min, the NMS's float32 IoU; among those the highest score, the lowest index on a tie.
 *   d_view_n     [B, cap] int32   the number of views with a witness
 *   d_view_bits  [B, cap] int32   bit v: view v has a witness
 *   d_view_score [B, cap] float   the float64 sum of the witnesses' scores in view order, / n_views (an absent witness counts 0),
 *                                 rounded once
 *   d_view_var   [B, cap, 4] float the population variance over the witnesses of (cx, cy, w, h), cx = (x0 + x1) 0.5, w = x1 - x0
 *                                 on the sorted corners: float64 on the float32 inputs, mean = sum / n in view order, then
 *                                 sum (c - mean)^2 / n in view order (no fused multiply-add), rounded once; 0 for n <= 1
 * all 0 in the padding (k >= count).  Deterministic; an image gives the same bytes at any position of any batch.
 * iou_min = 0.5 and min_score = 0.001 are starting values that nobody has tuned.  Refused with BYOLO_ERR_ARG, the field named: a
 * wrong struct_bytes, n_views outside 1 .. BYOLO_TTA_MAX_VIEWS, view_off not starting at 0, not ascending or beyond Nu, iou_min
 * negative or NaN, min_score NaN; a workspace below byolo_tta_support_workspace_bytes(B, Nu) is BYOLO_ERR_NOMEM. */
#define BYOLO_TTA_MAX_VIEWS 8
typedef struct byolo_tta_support_cfg {
    int32_t struct_bytes;          /* sizeof(byolo_tta_support_cfg) of the caller's header: a mismatch is BYOLO_ERR_ARG */
    int32_t n_views;
    float iou_min, min_score;
    int32_t view_off[BYOLO_TTA_MAX_VIEWS + 1];
} byolo_tta_support_cfg;
BYOLO_API int32_t byolo_tta_view_f32(const float* d_in, int32_t B, int32_t src_h, int32_t src_w, int32_t flip, int32_t out_h,
                                     int32_t out_w, float* d_out, void* stream);
BYOLO_API int32_t byolo_tta_merge(const float* d_rows, int32_t B, int64_t Nv, int32_t D, int32_t kind, int32_t layer_col, int32_t flip,
                                  int32_t size_idx, float* d_union, int64_t Nu, int64_t row_off, void* stream);
BYOLO_API size_t byolo_tta_support_workspace_bytes(int32_t B, int64_t Nu);
BYOLO_API int32_t byolo_tta_support(byolo_t* h, const float* d_union, int32_t B, int64_t Nu, int32_t D, int32_t obj_idx,
                                    int32_t cls_start_idx, int32_t nms_mode, const byolo_tta_support_cfg* cfg, const int32_t* d_kept,
                                    const int32_t* d_count, int32_t cap, int32_t* d_view_n, int32_t* d_view_bits, float* d_view_score,
                                    float* d_view_var, void* d_ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* BYOLO_H_ */
