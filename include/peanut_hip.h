/* peanut_hip -- C ABI of the MI355X-native PEANUT perception hot path (libpeanut_hip.so).
 *
 * The reference (ajzhai/PEANUT) has no plugin/FFI layer: its boundary for this path is three
 * Python call surfaces.  Each entry point below states the reference interface it replaces
 * (paths relative to the reference checkout).  Conventions:
 *   - every `const float* dev` / `float* dev` is a DEVICE pointer (e.g. torch.Tensor.data_ptr());
 *     the caller owns every buffer; `host` pointers are marked as such;
 *   - functions enqueue on the given hipStream_t (passed as void*; NULL = default stream) and do
 *     not synchronise unless stated;
 *   - return 0 on success, a negative PEANUT_E* code otherwise; peanut_last_error() returns a
 *     thread-local message for the last failure;
 *   - a handle is not thread-safe, distinct handles are; the process DEFAULTS of the tuning options (peanut_set_default_option) are
 *     one unlocked table that every peanut_*_create snapshots: callers that create handles on several threads while changing
 *     defaults serialise those calls themselves (the Python mirrors do, under one lock).
 */
#ifndef PEANUT_HIP_H_
#define PEANUT_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PEANUT_OK 0
#define PEANUT_EINVAL (-2)   /* bad argument / unsupported configuration */
#define PEANUT_EHIP (-3)     /* HIP runtime error */
#define PEANUT_EWEIGHTS (-4) /* missing or mis-shaped tensor in the state dict */
#define PEANUT_ERANGE (-5)   /* precision FP16X3: a value left fp16's exponent range (the result would be NaN / dropped) */

const char* peanut_last_error(void);
/* kernel family the calling thread's most recent conv / GEMM launch selected, e.g. "conv_pw_glds_256x128", "conv_pw_glds_256x256", "conv_pw_ares_128x128" (for tests
 * and profiles: lets a parity test assert which kernel produced the result it checked) */
const char* peanut_last_conv_kernel(void);
/* library / ABI version and the arch it was compiled for ("gfx950") */
int peanut_abi_version(void);
const char* peanut_build_arch(void);
/* hash of the sources this library was compiled from (peanut_amd/build.py: source_hash), "" when built by other means: the
 * Python binding compares it with the sources lying next to it and rebuilds or refuses a stale library */
const char* peanut_source_hash(void);
/* Host-side test hook (no GPU needed): the pieces the weight packer of an emulated mode makes of n host values that
 * form ONE layer -- precision = PEANUT_PREC_BF16X3 / FP16X3 (two pieces) or BF16X6 (three).  pieces: [3][n] 16-bit
 * patterns (bf16 or fp16; plane 2 zero for the two-piece modes); *pack_scale = the power of two the values were multiplied
 * by first (1 for the bf16 modes).  tests/test_abi.py compares them with numpy's / torch's own roundings. */
int peanut_debug_weight_pieces(const float* values, int n, int precision, unsigned short* pieces, float* pack_scale);
/* Host-side test hook (no GPU needed): the Winograd weight transform U = G g G^T of a [cout][cin][3][3] layer for output
 * tiles of tile x tile (4, 5 or 6; csrc/winograd.hip), as the uploader computes it (double arithmetic, rounded once):
 * out [(tile + 2)^2][cout][cin].  tests/test_abi.py holds it against the Toom-Cook construction in exact rationals. */
int peanut_debug_wino_weights(const float* w_oihw, int cout, int cin, int tile, float* out);
/* Test hook (ABI 14): how many Winograd input transforms of this process have summed their producer's split-K partial tiles
 * themselves (csrc/common.h DeferredSplit; option defer_splitk): a Bottleneck conv1 at batch 1 then runs no reduce launch.  Replaces
 * nothing in the reference (resnet.py:267-307 conv1 -> bn1 -> relu -> conv2 are four module calls there); lets a test assert
 * that the fused path really ran while the results stay bit-identical. */
long long peanut_debug_deferred_splitk_count(void);
/* Test hook (ABI 14): an LDS canary.  Enqueues `workgroups` workgroups of 256 threads on `stream`, each of which fills `lds_bytes`
 * (<= 64 KiB, a multiple of 1024) of its LDS with a pattern and then, `rounds` times, sleeps a little and checks it; words found
 * changed are counted into *mismatches (device pointer, int, the caller zeroes it).  Run next to another kernel on a second stream it
 * shows whether that kernel writes LDS outside its own allocation (a workgroup that shares the CU would see it).  rounds < 0: |rounds|
 * rounds without the sleep and with a sweep of broadcast 16-byte reads over the whole array in each -- an LDS-heavy neighbour.  Nothing in
 * the reference corresponds to it. */
int peanut_debug_lds_canary(int workgroups, int lds_bytes, int rounds, int* mismatches, void* stream);
/* Test hook (ABI 15): a packed-FMA canary.  Workgroups of 256 threads that compute, `rounds` times, twelve 64-term dot products per thread
 * three ways on the same operands, two sums per packed instruction: `v_pk_fma_f32 ... op_sel:[0,1,0]` (the shared operand in the HIGH
 * register of its pair: the form hipcc emits when it packs scalar code), `v_pk_fma_f32 ... op_sel_hi:[1,0,1]` (the operand in the LOW
 * register) and two scalar v_fmac_f32.  mismatches (device pointer, TWO ints, zeroed by the caller): [0] sums where the first form differs
 * from the scalar one, [1] where the second does.  The same arithmetic: any difference is the hardware.  Measured on gfx950 (profiles/r9r):
 * [0] > 0 while fp16 / bf16 MFMA waves share the SIMD (the emulated modes' GEMM kernels), 0 otherwise; [1] always 0. */
int peanut_debug_pkfma_canary(int workgroups, int rounds, int* mismatches, void* stream);

/* ------------------------------------------------------------------------------------------
 * Tuning options (csrc/options.h): kernel gates, Winograd form policy, launch-plan switches -- named by key, e.g.
 * "pw256_mink"; peanut_option_list() returns one line per option: `key=default [create-time] help`.
 * The process defaults come from the PEANUT_<KEY> environment variables (read once) and peanut_set_default_option.  A
 * handle (peanut_pred_t / peanut_conv_t / peanut_rcnn_t) SNAPSHOTS the defaults when it is created and carries its own
 * copy: peanut_*_set_option changes that one handle (and drops its cached launch plans), so two handles in one process
 * can run different policies.  Options marked [create-time] shape the uploaded weights (Winograd forms, packing tiles):
 * set them as defaults before the create call; peanut_*_set_option refuses them.
 * ---------------------------------------------------------------------------------------- */
int peanut_set_default_option(const char* key, long long value);
int peanut_get_default_option(const char* key, long long* value);
const char* peanut_option_list(void);

/* ------------------------------------------------------------------------------------------
 * Stage 3 -- map-completion forward (PSPNet: ResNet-50-V1c-D8 + PSP head)
 * ---------------------------------------------------------------------------------------- */

/* Fields of nav/pred_model_cfg.py:2-42 that the inference path reads. */
typedef struct peanut_pred_cfg {
  int in_channels;       /* backbone.in_channels (14) */
  int num_classes;       /* decode_head.num_classes (6) */
  int strides[4];        /* backbone.strides (1,2,1,1) */
  int dilations[4];      /* backbone.dilations (1,1,2,4) */
  int contract_dilation; /* backbone.contract_dilation (True) */
  int pool_scales[8];    /* decode_head.pool_scales (1,2,3,6) */
  int n_pool_scales;
  int head_channels;     /* decode_head.channels (512) */
  int align_corners;     /* decode_head.align_corners (False) */
  float bn_eps;          /* nn.BatchNorm2d default 1e-5 */
  int precision;         /* PEANUT_PREC_*: arithmetic of the conv contractions (see below) */
  int fold_ppm;          /* 1: evaluate the pyramid half of the PSP bottleneck conv through linearity
                            (conv of a bilinear upsample of k*k vectors = bilinear blend of k*k folded
                            vectors; halves that conv's FLOPs, fp32 re-association only); 0: plain conv */
  int conv_algo;         /* PEANUT_ALGO_*: algorithm of the stride-1 3x3 convs with >= 64 input channels */
} peanut_pred_cfg;

/* PEANUT_ALGO_AUTO: Winograd with fp32 transforms, the form chosen per layer and shape -- F(6x6,3x3), F(5x5,3x3) (dilation-4
 * layers of the prediction backbone) or F(4x4,3x3) in the prediction model and the detector's front end, F(4x4,3x3) for
 * single convs, the detector heads and the PSP bottleneck of the emulated modes -- (what cuDNN/MIOpen pick for these layers
 * in the reference's own GPU runs): 4x / 4.6x / 5.1x fewer multiplies; well-conditioned interpolation points (0, +-3/4,
 * +-3/2, inf; 0, +-1/2, +-1, 3, inf; 0, +-1/2, +-1, +-2, inf) and position GEMMs that accumulate in two levels on the fp32
 * kernels (partial sums of 64 channels) keep the logits within 1e-5 max-abs of the reference golden vectors (direct form
 * 9e-6, bound 1e-3).
 * AUTO also runs conv3 and a stride-1 downsample / shortcut conv of a bottleneck block as ONE GEMM over [conv2 output | block
 * input] with the two BatchNorm scales folded into the weights (same function, another rounding order).
 * PEANUT_ALGO_DIRECT: every conv as the direct implicit GEMM (products summed exactly as an fmaf chain), every block in
 * the reference's op-for-op form (conv -> BN, conv -> BN, add, ReLU). */
#define PEANUT_ALGO_AUTO 0
#define PEANUT_ALGO_DIRECT 1

/* Conv arithmetic.  FP32: v_mfma_f32_32x32x2_f32 -- exact fp32 products, fp32 accumulation.  The pointwise GEMM families sum
 * a layer's products in ONE order and agree bit for bit with each other and with an fmaf chain in that order (only a tail
 * split-K cuts K differently by tile size); the summation order of the other kernels is kernel-dependent: the LDS-patch stem
 * kernel (csrc/conv_patch.hip) keeps two accumulator chains, the Winograd position GEMMs accumulate in two levels, and the
 * row groups of the pyramid pooling (option ppm_group_rows = 0: chosen from H * B, so that ~768 workgroups run) make the last
 * bits of the PSP pooling sums depend on the BATCH SIZE as well as on the position in the batch -- all within ~1e-6 relative.
 * BF16X6: fp32 emulated on the bf16 matrix cores.  Activations stay fp32 in HBM and LDS -- the forward's tensors,
 * Winograd transforms and fusions are exactly the fp32 mode's; every fp32 value is split into three bf16 pieces (3 x 8 =
 * 24 mantissa bits: the split is exact; the activations in registers after the fragment read, the weights once at load
 * time) and every product is rebuilt from the six piece products that matter (hi*hi, hi*mid, mid*hi, mid*mid, hi*lo,
 * lo*hi; the dropped ones are <= 2^-24 relative, the size of fp32's own product rounding) on v_mfma_f32_32x32x16_bf16
 * with fp32 accumulation: fp32-class results, measured as close to a float64 run of the reference model as the
 * reference's own fp32 CPU path.  The 1x1 convs and the Winograd position GEMMs run on csrc/gemm_rs.hip, every other conv
 * (3x3 direct, strided, the stem) on csrc/conv_rs.hip -- the same arithmetic with im2col-free staging; the Winograd
 * transforms themselves are fp32 in every mode.
 * BF16X3: the same with two pieces and three products (~2^-16 relative per product: ~7e-5 max-abs on the logits,
 * bound 1e-3); an opt-in speed mode, not fp32-class.
 * FP16X3: two FP16 pieces per value (2 x 11 = 22 significand bits) and the three products hi*hi, hi*lo, lo*hi on
 * v_mfma_f32_32x32x16_f16 with fp32 accumulation -- the cost of BF16X3 at close to BF16X6's accuracy (dropped / rounded
 * terms <= 2^-21.5 relative per product).  What it gives up is fp32's exponent range in the ACTIVATIONS of the emulated
 * layers: they must stay below 65504 in magnitude (Winograd-domain values included), and the low piece of a value below
 * 2^-3 is an fp16 subnormal (absolute error <= 3e-8, fp32's own rounding of a value near 0.5).  Weights are scaled by a
 * per-layer power of two before the split (undone exactly in the epilogue), so their range does not matter.  Opt-in. */
#define PEANUT_PREC_FP32 0
#define PEANUT_PREC_BF16X3 1
#define PEANUT_PREC_FP16X3 2
#define PEANUT_PREC_BF16X6 3

/* One entry of an mmcv/PyTorch state dict (HOST memory, fp32, contiguous, OIHW for convs). */
typedef struct peanut_tensor {
  const char* name;  /* e.g. "backbone.layer1.0.conv1.weight" */
  const float* data; /* host */
  int ndim;
  int64_t shape[4];
} peanut_tensor;

typedef struct peanut_pred peanut_pred_t;

/* Replaces init_segmentor (prediction/mmseg/apis/inference.py:12-40) as called from
 * PEANUT_Prediction_Model.__init__ (nav/agent/prediction.py:142-152): builds the layer table
 * from cfg, looks every tensor up BY NAME in the mmcv state-dict key schema
 * (auxiliary_head.* and num_batches_tracked entries are ignored), folds BatchNorm into a
 * per-channel scale/shift, repacks conv weights into the kernel tile layout and uploads them.
 * Synchronous. */
int peanut_pred_create(peanut_pred_t** out, const peanut_pred_cfg* cfg, const peanut_tensor* tensors,
                       int n_tensors);
void peanut_pred_destroy(peanut_pred_t* h);

/* Replaces run_inference + model(return_loss=False, rescale=True) + (optionally) expit:
 * nav/agent/prediction.py:112-137,155-158 -> prediction/mmseg/models/segmentors/
 * encoder_decoder.py:70-80,203-271.  in_dev: [B, in_channels, H, W] NCHW fp32;
 * out_dev: [B, num_classes, H, W] NCHW fp32 raw logits (apply_sigmoid=0, what simple_test
 * returns in the fork) or probabilities (apply_sigmoid=1, what get_prediction returns).
 * The activation workspace for a (B,H,W) shape is allocated on first use and cached. */
int peanut_pred_forward(peanut_pred_t* h, const float* in_dev, float* out_dev, int B, int H, int W,
                        int apply_sigmoid, void* stream);

/* Bytes of activation workspace a (B,H,W) forward needs (0 on error). */
size_t peanut_pred_workspace_bytes(peanut_pred_t* h, int B, int H, int W);

/* Conv FLOPs (2 x MACs over the 61 convolutions) of one HxW map. */
double peanut_pred_flops_per_map(peanut_pred_t* h, int H, int W);

/* Sliding-window and flip-averaged inference (ABI 24; csrc/pred_infer.hip): what the reference's EncoderDecoder does around its
 * forward when nav/pred_model_cfg.py says test_cfg.mode='slide' or the test pipeline's MultiScaleFlipAug says flip=True --
 * slide_inference (prediction/mmseg/models/segmentors/encoder_decoder.py:155-201), the flip branch of inference() (:249-256) and
 * the averaging of aug_test (:273-291), reached through BaseSegmentor.forward_test (segmentors/base.py:62-110) with the images
 * MultiScaleFlipAug builds (datasets/pipelines/test_time_aug.py:102-135).  Arguments as a descriptor; the stream the work is
 * enqueued on travels in it (NULL = default stream).
 *   Window grid (:166-177, per axis): grids = max(n - crop + stride - 1, 0) / stride + 1; window i ends at min(i * stride + crop, n)
 * and starts at max(end - crop, 0): a ragged last window is shifted back, and a crop larger than the image gives the one window
 * min(crop, n) ("the small patch will be used").  Whole mode is the one window (0, 0, H, W).
 *   Three steps: ONE launch gathers every window of every flipped image into a staged batch [N, C, ch, cw], N = n_augs * B * windows,
 * ordered aug-major, then sample, then window row-major (the flip is applied to the whole image before the windows are cut, as the
 * pipeline's np.flip does); the forward of peanut_pred_forward -- raw logits at window resolution, never the hipGraph replay -- runs
 * over the staged batch in chunks of max_batch maps; ONE launch combines.  The rule of the combine, held bit for bit:
 *     per aug a:  s = +0.0f;  s = s + logit for every window that covers the pixel, in row-major window order;
 *                 slide: p_a = s / (float)count (an IEEE division);  whole: p_a = the logit;  p_a is then un-flipped;
 *     out = p_0;  out = out + p_a for a = 1.. in order;  if n_augs > 1: out = out / (float)n_augs (simple_test does not divide);
 *     then the optional sigmoid (apply_sigmoid = 1).
 * The final resize of :195-200 / :216-221 is at ratio 1.0 (img_ratios other than [1.0] are refused by the config reader) and is the
 * identity: it is not launched.  The last bits of a logit depend on the batch size of its forward (see "Conv arithmetic" below),
 * hence on max_batch.  in_dev: [B, in_channels, H, W] NCHW fp32; out_dev: [B, num_classes, H, W], written whole.  The staging
 * buffers are allocated on first use and cached on the handle, like the activation workspace (growing them frees the old ones).
 * No synchronisation: the window grid is host arithmetic and nothing is read back.  PEANUT_EINVAL with nothing enqueued: a null
 * pointer, B < 1, a mode other than 0 / 1, slide mode with a crop or stride below 1, a pixel that no window covers (stride > crop:
 * the reference asserts on it), more than PEANUT_INFER_MAX_GRID windows on an axis, an effective window below the forward's
 * minimum of 16, n_augs outside 1..PEANUT_INFER_MAX_AUGS, a flip code outside 0..2, max_batch < 0, out_dev overlapping in_dev, a
 * handle under the event probe. */
#define PEANUT_INFER_MAX_AUGS 4
#define PEANUT_INFER_MAX_GRID 32           /* windows per axis */
typedef struct {
  int mode;                                /* 0 whole, 1 slide */
  int crop_h, crop_w, stride_h, stride_w;  /* slide: test_cfg.crop_size / .stride, (h, w) */
  int n_augs;                              /* 1 .. 4: the images forward_test is handed */
  int flip[PEANUT_INFER_MAX_AUGS];         /* per aug: 0 none, 1 horizontal (dims=(3,)), 2 vertical (dims=(2,)) */
  int max_batch;                           /* most maps per internal forward; 0 = all of them in one */
  void* stream;
} peanut_pred_infer_t;
int peanut_pred_inference(peanut_pred_t* h, const peanut_pred_infer_t* infer, const float* in_dev, float* out_dev,
                          int B, int H, int W, int apply_sigmoid);
/* The window grid of a descriptor on an H x W image, host only: y1 / x1 (each int[PEANUT_INFER_MAX_GRID], may be NULL) receive the
 * per-axis window starts (the grid is separable; entries past the axis' count are -1), *ch / *cw the effective window size
 * min(crop, n).  Returns h_grids * w_grids, or PEANUT_EINVAL for everything peanut_pred_inference refuses that needs no handle. */
int peanut_pred_infer_windows(const peanut_pred_infer_t* infer, int H, int W, int* y1, int* x1, int* ch, int* cw);
/* Bytes the call needs on the handle: the two staging buffers and the activation workspace of its largest forward (0 on error). */
size_t peanut_pred_inference_workspace_bytes(peanut_pred_t* h, const peanut_pred_infer_t* infer, int B, int H, int W);
/* The two glue launches of peanut_pred_inference on the caller's buffers, no handle (tests and tools/bench_infer.py time them alone;
 * a caller with a forward of its own can put it between them).  Gather: in_dev [B, C, H, W] -> staged_dev [N, C, ch, cw] in the
 * order above.  Combine: logits_dev [N, K, ch, cw] in that order -> out_dev [B, K, H, W] by the rule above.  One launch each on
 * infer->stream.  No synchronisation, no allocation.  PEANUT_EINVAL with nothing enqueued: as peanut_pred_infer_windows; a null
 * pointer; B, C or K below 1; source and destination overlapping. */
int peanut_pred_infer_gather(const peanut_pred_infer_t* infer, const float* in_dev, float* staged_dev, int B, int C, int H, int W);
int peanut_pred_infer_combine(const peanut_pred_infer_t* infer, const float* logits_dev, float* out_dev, int B, int K, int H, int W,
                              int apply_sigmoid);

/* Test/bisect hook: keep every intermediate of subsequent forwards in its own buffer
 * (keep=1) and fetch one by name after a forward.  Names: "stem0","stem1","stem2","pool",
 * "layer1".."layer4","ppm_table","bottleneck","logits_lowres".  *dev_out points into the
 * handle's workspace (NHWC; dims = {B,H,W,C}; "ppm_table" is {B,1,nbins,C}). */
int peanut_pred_debug_keep(peanut_pred_t* h, int keep);
int peanut_pred_debug_tensor(peanut_pred_t* h, const char* name, const float** dev_out, int dims[4]);
/* Same lookup, but copies the tensor into dst_dev (device, >= max_floats capacity) on `stream`;
 * dst_dev == NULL only reports dims. */
int peanut_pred_debug_read(peanut_pred_t* h, const char* name, float* dst_dev, size_t max_floats, int dims[4],
                           void* stream);

/* Event probe (used by bench.py for the roofline figure): while enabled, every forward records a
 * HIP event before/after each launch ON THE STREAM THE KERNELS RUN ON.  collect() synchronises
 * on those events, sums each op's elapsed time over all forwards since the last collect and
 * clears the probe.  names/kernels point to storage owned by the handle (valid until the plan
 * is dropped); kernels[i] is the kernel family op i launches (e.g. "conv_pw_glds_128x128"): the
 * plan takes it from the same route the launch takes, and a forward under the probe fails with
 * PEANUT_EINVAL (both names in the message) if a conv op's launch recorded another family;
 * flops[i] = FLOPs one launch of op i executes; bytes[i] = its algorithmic HBM bytes (every operand read
 * once, the result written once).  Returns the op count. */
int peanut_pred_probe_enable(peanut_pred_t* h, int enable);
int peanut_pred_probe_collect(peanut_pred_t* h, int max_ops, const char** names, const char** kernels,
                              double* ms_sum, double* flops, double* bytes, int* n_forwards);
/* hipGraph replay: with enable = 1 the launch sequence of a (B,H,W, in, out, apply_sigmoid, stream) combination is
 * captured on its second use and replayed as ONE hipGraphLaunch afterwards (~85 kernels per forward; measured on
 * MI355X the small-batch cases are bound by the dependent chain on the device, not by launches: no gain).
 * Up to 16 combinations are cached; growing the workspace drops them.  Results are identical.  Ignored while the probe or debug taps are on, and on the legacy default stream (NULL), which HIP
 * cannot capture: pass a created stream. */
int peanut_pred_use_graph(peanut_pred_t* h, int enable);
/* Tuning options of this handle (see above).  Not while the probe is enabled. */
int peanut_pred_set_option(peanut_pred_t* h, const char* key, long long value);
int peanut_pred_get_option(peanut_pred_t* h, const char* key, long long* value);

/* ------------------------------------------------------------------------------------------
 * Stage 2 -- egocentric -> allocentric semantic-map projection
 * ---------------------------------------------------------------------------------------- */

/* The `args` fields Semantic_Mapping.__init__ reads (nav/agent/mapping.py:15-37); python floats are
 * doubles here and are narrowed to fp32 exactly where torch narrows them. */
typedef struct peanut_map_cfg {
  int frame_height, frame_width;   /* 120, 160 */
  int map_resolution;              /* 5 (cm per cell) */
  int map_size_cm;                 /* 4800 */
  int global_downscaling;          /* 2 */
  int vision_range;                /* 100 */
  double hfov;                     /* 79.0 */
  int du_scale;                    /* 1 (1..8: depth pixels taken every du_scale-th row / column, depth_utils.py:129-149) */
  double cat_pred_threshold, exp_pred_threshold, map_pred_threshold;   /* 5.0, 1.0, 0.1 */
  int num_sem_categories;          /* 10 */
  double camera_height;            /* 0.88 (m) */
} peanut_map_cfg;

typedef struct peanut_map peanut_map_t;

/* Replaces Semantic_Mapping.__init__ (mapping.py:12-50): derives the constants (camera matrix,
 * z bins, paste window) and allocates the per-frame scratch (a few MB).  Synchronous. */
int peanut_map_create(peanut_map_t** out, const peanut_map_cfg* cfg);
void peanut_map_destroy(peanut_map_t* h);
/* dims = {C (= 4 + num_sem_categories), M (local map cells), vision_range, frame points} */
int peanut_map_dims(peanut_map_t* h, int dims[4]);

/* Replaces Semantic_Mapping.forward (mapping.py:52-179) for batch size 1.  All pointers are device
 * fp32: obs [1,C,h,w] (ch 3 = depth in cm, ch 4.. = semantic), pose_obs [3] = (dx, dy, dtheta),
 * maps_last [C,M,M], poses_inout [3] = (x m, y m, theta deg) updated IN PLACE (the reference's
 * returned pose_pred / current_poses both alias poses_last, mapping.py:143-160), fp_map_pred
 * [1,V,V], map_pred [C,M,M] (must not alias maps_last).  Enqueues 7 launches (all own kernels; the points are grouped by voxel without a sort:
 * count, claim a segment, fill, rank inside the segment), no host sync. */
int peanut_map_forward(peanut_map_t* h, const float* obs, const float* pose_obs, const float* maps_last,
                       float* poses_inout, float* fp_map_pred, float* map_pred, void* stream);
/* The bookkeeping Agent_State.update_local_map does on the local map after the projection
 * (nav/agent/agent_state.py:281-296), in one launch instead of eight small tensor operations:
 *   local_map[2, :, :] = 0;  local_map[2:4, r0:r1, c0:c1] = 1  (the trajectory square `loc - 2 : loc + 3`, passed as the
 *   NORMALISED Python slice, 0 <= r0, r1 <= m; empty when r0 >= r1);  local_map[1][selem_rows + cr, selem_cols + cc] = 1 for
 *   up to two centres (the agent's cell; the current goal when the agent is within goal_reached_dist of it), where the
 *   footprint is the non-zero cells of selem (device uint8 [(2R+1), (2R+1)], `disk(col_rad + 1)`) offset by -R.  Negative
 *   indices wrap like torch's; a footprint index outside [-m, m) is refused (PEANUT_EINVAL; torch raises IndexError).
 * local_map: device fp32 [channels, m, m], channels >= 4.  No host sync. */
int peanut_map_mark_agent(float* local_map, int channels, int m, int r0, int r1, int c0, int c1, const uint8_t* selem,
                          int selem_radius, int n_centres, const int* centres_rc, void* stream);
/* hipGraph replay of the step's launches, keyed on the seven pointer/stream arguments (an agent ping-pongs two map
 * buffers: two cached graphs).  Applies to peanut_map_forward only: the batched call below always enqueues plainly. */
int peanut_map_use_graph(peanut_map_t* h, int enable);

/* ---- several episodes per step (the reference runs one process per environment on a shared card, nav/collect.py:32-50) ---- */
#define PEANUT_MAP_MAX_BATCH 16
/* Allocates max_batch (1..PEANUT_MAP_MAX_BATCH) slots of the per-frame scratch that the create call allocates once, each
 * initialised as that one is; a call with max_batch at or below what is reserved does nothing.  The slots are separate
 * from the single step's scratch, so single and batched steps on one handle do not disturb each other.  Synchronous:
 * all of the batched path's allocation happens here, none while stepping. */
int peanut_map_reserve(peanut_map_t* h, int max_batch);
/* Semantic_Mapping.forward (mapping.py:52-179) for E independent episodes in the launches of ONE single-episode step (8;
 * 9 with du_scale > 1): the episode is a grid dimension and every kernel runs the single step's own code on that
 * episode's scratch slot, so per episode every output is bit-identical to the single-episode call above on the same inputs.
 * obs [E,C,h,w], pose_obs [E,3], poses_inout [E,3] (in place), fp_map_pred [E,V,V]: device fp32, contiguous.  maps_last /
 * map_pred: HOST arrays of E device pointers, each [C,M,M] (every episode owns its map tensors; they go to the kernels by
 * value).  Refused with PEANUT_EINVAL, nothing enqueued: E above the reserved batch, a null pointer, a map_pred that is
 * also some episode's maps_last, two episodes sharing one map_pred.  No host sync, no graph replay. */
int peanut_map_forward_batch(peanut_map_t* h, int E, const float* obs, const float* pose_obs, const float* const* maps_last,
                             float* poses_inout, float* fp_map_pred, float* const* map_pred, void* stream);
/* The bookkeeping of the single-map call above (nav/agent/agent_state.py:281-296) for E maps in one launch.  local_maps: host
 * array of E distinct device pointers, each [channels, m, m]; squares: host [E,4] = (r0, r1, c0, c1) per episode; n_centres:
 * host [E]; centres_rc: host [E,2,2].  The single call's checks are applied to every episode before anything is enqueued:
 * one refused episode refuses the whole call and leaves every map as it was. */
int peanut_map_mark_agent_batch(int E, float* const* local_maps, int channels, int m, const int* squares, const uint8_t* selem,
                                int selem_radius, const int* n_centres, const int* centres_rc, void* stream);
/* Test hook: kernels enqueued by the handle's most recent forward call, single or batched (counted on the host beside the
 * launches); -1 for a null handle. */
int peanut_map_debug_launches(peanut_map_t* h);

/* ---- the goal map of the planner inputs (Agent_State.update_goal_map, nav/agent/agent_state.py:418-446) ----
 * Whether the agent has seen its object, and the goal cells handed to the planner.  Stateless; two launches (the morphology per
 * 32 x 32 tile in LDS, then one workgroup per episode that forms the flag and marks the goal cell), no host sync.
 *   S = local_map[cn] > 0                     (the projection keeps the map non-negative, so this is the reference's `> 0` AND makes
 *                                              its early-out `local_map[cn].sum() != 0` redundant: a zero sum leaves S empty)
 *   if morph: S eroded n_erode times, then dilated once (also when n_erode = 0); 4-connected cross; cells outside the map are SET
 *             for the erosion and UNSET for the dilation (scipy.ndimage.binary_erosion(border_value=1) / binary_dilation, which
 *             is what scikit-image's binary_erosion / binary_dilation call)
 *   S &= ((((((c4 + c5) + c6) + c7) + c8) + c9) - c[cn]) == 0     fp32, in that order, over the planes 4 .. min(10, channels) - 1
 *                                                                 (the reference's hard-coded 4:10), AFTER the morphology
 *   found = any(S);  goal_map = S if found, else zero but for goal_map[goal_r, goal_c] = 1.  detect = 0 (only_explore): always the latter.
 * local_map: device fp32, `channels` planes of m x m, plane_stride / row_stride in ELEMENTS, column stride 1 -- a view into the
 * full map is read in place; it is never written.  cn: 4 <= cn < channels.  morph, detect: 0 or 1 (morph = the goal is not a tv).
 * n_erode: 0..PEANUT_GOAL_MAP_MAX_ERODE (args.goal_erode, 3 in the reference).  goal_r, goal_c in [0, m).  goal_map: device uint8
 * [m, m], contiguous; found: device int32.  Both are written completely whatever they held.  PEANUT_EINVAL, nothing enqueued: a
 * null pointer, a value outside the ranges above, strides under which planes or rows would overlap. */
#define PEANUT_GOAL_MAP_MAX_ERODE 8
int peanut_goal_map(const float* local_map, int channels, int m, long long plane_stride, long long row_stride, int cn, int morph,
                    int n_erode, int detect, int goal_r, int goal_c, uint8_t* goal_map, int32_t* found, void* stream);
/* The same for E episodes (1..PEANUT_MAP_MAX_BATCH) in the same two launches, the episode being a grid dimension: every episode's
 * goal_map and found[e] are the bits of the single call.  local_maps, goal_maps: HOST arrays of E device pointers; plane_strides,
 * row_strides: host [E]; params: host [E,6] = (cn, morph, n_erode, detect, goal_r, goal_c) per episode; found: DEVICE int32 [E].
 * The single call's checks are applied to every episode before anything is enqueued; two episodes whose goal maps overlap
 * (the byte ranges [goal_map, goal_map + m * m), identical pointers included) are refused too.  One refused episode refuses the
 * whole call and leaves every output as it was.  Not checked, in either call: a goal_map or found that lies inside a local map or
 * inside each other -- the outputs are the caller's own buffers, apart from every input. */
int peanut_goal_map_batch(int E, const float* const* local_maps, int channels, int m, const long long* plane_strides,
                          const long long* row_strides, const int* params, uint8_t* const* goal_maps, int32_t* found, void* stream);

/* ------------------------------------------------------------------------------------------
 * Stage 1 -- Mask R-CNN front end (preprocessing + ResNet-FPN backbone + RPN head)
 *
 * Replaces the dense-convolution part of detectron2's DefaultPredictor as built by
 * SemanticPredMaskRCNN.__init__ (nav/agent/utils/segmentation.py:30-38) from
 * COCO-InstSeg/mask_rcnn_R_101_cat9.yaml.  detectron2 is third party and absent from the reference
 * checkout: the module graph follows its published v0.6 definitions, parity is pinned only against
 * the restatement in oracle/rcnn_ref.py.  Proposal selection, NMS, ROIAlign and mask pasting are the operator
 * exports further down; peanut_rcnn_inference runs the whole detector.
 * ---------------------------------------------------------------------------------------- */
typedef struct peanut_rcnn_cfg {
  int depth;               /* RESNETS.DEPTH (101) */
  int stem_out;            /* RESNETS.STEM_OUT_CHANNELS (64) */
  int res2_out;            /* RESNETS.RES2_OUT_CHANNELS (256) */
  int stride_in_1x1;       /* RESNETS.STRIDE_IN_1X1 (true) */
  int fpn_out;             /* FPN.OUT_CHANNELS (256) */
  int num_anchors;         /* len(ANCHOR_GENERATOR.ASPECT_RATIOS[0]) (3) */
  int min_size, max_size;  /* INPUT.MIN_SIZE_TEST / MAX_SIZE_TEST (800, 1333) */
  int size_divisibility;   /* 32 */
  float pixel_mean[3], pixel_std[3]; /* BGR (103.53, 116.28, 123.675), (1, 1, 1) */
  float bn_eps;            /* FrozenBatchNorm2d eps 1e-5 */
  int precision;           /* PEANUT_PREC_* */
  int conv_algo;           /* PEANUT_ALGO_* (Winograd for the stride-1 3x3 convs with >= 128 input channels) */
  /* proposal generator and ROI heads (yaml :41-57, :163-253, :312); read by peanut_rcnn_inference only */
  float anchor_sizes[5];   /* ANCHOR_GENERATOR.SIZES, one per level p2..p6 (32, 64, 128, 256, 512) */
  float aspect_ratios[8];  /* ANCHOR_GENERATOR.ASPECT_RATIOS (0.5, 1, 2): num_anchors entries */
  int rpn_pre_nms_topk;    /* RPN.PRE_NMS_TOPK_TEST (1000; <= 1024) */
  int rpn_post_nms_topk;   /* RPN.POST_NMS_TOPK_TEST (1000) */
  float rpn_nms_thresh;    /* RPN.NMS_THRESH (0.7) */
  float rpn_bbox_weights[4];   /* RPN.BBOX_REG_WEIGHTS (1, 1, 1, 1) */
  int num_classes;         /* ROI_HEADS.NUM_CLASSES (9) */
  int box_pooler_resolution, mask_pooler_resolution;   /* 7, 14 */
  int fc_dim;              /* ROI_BOX_HEAD.FC_DIM (1024), NUM_FC 2 */
  int mask_conv_dim, num_mask_convs;                   /* ROI_MASK_HEAD.CONV_DIM (256), NUM_CONV (4) */
  float roi_bbox_weights[4];   /* ROI_BOX_HEAD.BBOX_REG_WEIGHTS (10, 10, 5, 5) */
  float score_thresh_test; /* ROI_HEADS.SCORE_THRESH_TEST (segmentation.py:33 sets it to sem_pred_prob_thr) */
  float nms_thresh_test;   /* ROI_HEADS.NMS_THRESH_TEST (0.5) */
  int detections_per_image;    /* TEST.DETECTIONS_PER_IMAGE (100) */
  float mask_threshold;    /* detector_postprocess (0.5) */
} peanut_rcnn_cfg;

typedef struct peanut_rcnn peanut_rcnn_t;

/* tensors: detectron2 state-dict entries (host fp32), names like "backbone.bottom_up.res4.7.conv2.weight",
 * "....conv2.norm.running_var", "backbone.fpn_lateral3.bias", "proposal_generator.rpn_head.conv.weight". */
int peanut_rcnn_create(peanut_rcnn_t** out, const peanut_rcnn_cfg* cfg, const peanut_tensor* tensors, int n_tensors);
void peanut_rcnn_destroy(peanut_rcnn_t* h);
int peanut_rcnn_set_option(peanut_rcnn_t* h, const char* key, long long value);
/* Geometry of a (B,H,W) input: resized (h,w), zero-padded (h,w), the 5 pyramid level sizes p2..p6 as
 * level_hw = {h2,w2,...,h6,w6}, workspace bytes, conv FLOPs per image.  Any output may be NULL. */
int peanut_rcnn_plan(peanut_rcnn_t* h, int B, int H, int W, int resized_hw[2], int padded_hw[2], int level_hw[10],
                     size_t* workspace_bytes, double* flops_per_image);
/* img_bgr: device uint8 [B,H,W,3] (what DefaultPredictor receives, segmentation.py:44-45).  Outputs
 * (device fp32 NHWC, each array has 5 entries for p2..p6, entries or whole arrays may be NULL):
 * pyramid[l] [B,h_l,w_l,fpn_out], objectness[l] [B,h_l,w_l,A], deltas[l] [B,h_l,w_l,4A].
 * The RPN head runs on all five levels as ONE chain (five Winograd input transforms, one grouped position GEMM, five output
 * transforms, one objectness and one anchor-delta GEMM over all levels' rows: 12 launches instead of 25; option rcnn_rpn_fused)
 * whenever objectness[0..4] -- and deltas[0..4] -- are consecutive pieces of ONE buffer in level order (objectness[l + 1] ==
 * objectness[l] + B*h_l*w_l*A), or are not asked for; scattered buffers get the level-by-level launches.  The small levels may
 * then take another Winograd tile size than on their own: results agree to ~1e-5. */
int peanut_rcnn_forward_front(peanut_rcnn_t* h, const uint8_t* img_bgr, int B, int H, int W, float* const* pyramid,
                              float* const* objectness, float* const* deltas, void* stream);

/* Event probe of the front end (bench.py: stage-1 roofline): runs it `reps` times on `stream` with a HIP event after every
 * op, synchronises, and reports per op its name, the kernel family the launch picked (peanut_last_conv_kernel; "wino+..."
 * = Winograd transforms + that GEMM), the mean milliseconds and the direct-form conv FLOPs (0 for non-conv ops).  Fails with
 * PEANUT_EINVAL if a conv op ran another family than its plan names (the route of csrc/conv_route.hip, asked twice).  names /
 * kernels point to storage owned by the handle (valid until the next probe or plan change).  Returns the op count. */
int peanut_rcnn_probe_front(peanut_rcnn_t* h, const uint8_t* img_bgr, int B, int H, int W, int reps, int max_ops,
                            const char** names, const char** kernels, double* ms, double* flops, void* stream);

/* Stage timing of peanut_rcnn_inference / peanut_rcnn_semantic (bench.py: the roofline of stage 1's BACK half -- proposal
 * selection, ROI heads, mask paste: nav/agent/utils/segmentation.py:41-62 around detectron2's GeneralizedRCNN.inference).  While
 * enabled, every call records a HIP event on its stream at the nine stage boundaries: front_end | rpn_selection | roi_align_7x7 |
 * box_head_fc | box_postprocess_nms | host_read_detection_counts | roi_align_14x14 | mask_head_convs | mask_probabilities_paste
 * (a call without detections ends after the sixth).  peanut_rcnn_stage_times reports, for the LAST call, each stage's name, the
 * roof that bounds it ("mfma" | "hbm" | "host"; static strings), its milliseconds and its algorithmic work (FLOPs for "mfma"
 * stages -- the front end's are the direct-form count of its convs (nominal: its Winograd layers execute fewer), the heads'
 * are the executed ones; bytes with every operand read once and every result written once for "hbm" stages); returns the
 * stage count. */
int peanut_rcnn_set_stage_timing(peanut_rcnn_t* h, int on);
int peanut_rcnn_stage_times(peanut_rcnn_t* h, int max_stages, const char** names, const char** bounds, double* ms, double* work);

/* The detector's input transform alone (DefaultPredictor.__call__: ResizeShortestEdge.get_transform(img).apply_image,
 * i.e. PIL.Image.resize(BILINEAR) for uint8 frames -- Pillow's two-pass fixed-point resample, restated bit for bit --
 * then GeneralizedRCNN.preprocess_image: (x - PIXEL_MEAN) / PIXEL_STD, zero padding to the size-divisible canvas).
 * img_bgr: device uint8 [B,H,W,3]; out_nchw: device float [B,3,Hp,Wp] (Hp, Wp from peanut_rcnn_plan).  The front end
 * computes the same pixels internally (in the layout its stem wants); this export exists for bisecting and parity. */
int peanut_rcnn_preprocess(peanut_rcnn_t* h, const uint8_t* img_bgr, int B, int H, int W, float* out_nchw, void* stream);

/* The whole detector: what `DefaultPredictor(img)["instances"]` yields (nav/agent/utils/segmentation.py:45) --
 * GeneralizedRCNN.inference + detector_postprocess as configured by mask_rcnn_R_101_cat9.yaml -- for a batch of frames.
 * Needs a handle created with the roi_heads.* tensors in the state dict (box_head.fc1/fc2, box_predictor.cls_score /
 * bbox_pred, mask_head.mask_fcn1..N / deconv / predictor).  img_bgr: device uint8 [B,H,W,3].  Outputs: n_det_host
 * [B] (HOST ints: detections per image, at most detections_per_image each); the detections of all images back to
 * back, image-major, in decreasing score order inside an image: boxes device [sum n, 4] (x0, y0, x1, y1 in pixels of
 * the ORIGINAL frame), scores device [sum n], classes device int32 [sum n], masks device uint8 [sum n, H, W] (1 where
 * the pasted mask >= mask_threshold; pass NULL to skip the mask head).  The caller sizes the buffers for
 * B * detections_per_image instances.  Synchronises the stream once (to read the detection counts).  With precision
 * FP16X3 the RPN objectness, class scores, box deltas and mask logits are scanned for non-finite values and the call
 * returns PEANUT_ERANGE instead of an image without detections (one more 4-byte read behind the mask head). */
int peanut_rcnn_inference(peanut_rcnn_t* h, const uint8_t* img_bgr, int B, int H, int W, int* n_det_host, float* boxes,
                          float* scores, int32_t* classes, uint8_t* masks, void* stream);
/* SemanticPredMaskRCNN.get_prediction (nav/agent/utils/segmentation.py:41-62) for a batch of frames: the detector as
 * above, then `semantic_input[:, :, cls] += pred_masks[j] * 1.` for every instance with cls in range(n_cats), score >=
 * sem_pred_prob_thr and, for the frame's goal category, score >= goal_thr -- evaluated per output pixel straight from
 * the 28 x 28 mask probabilities (same arithmetic as peanut_paste_masks), so the [n,H,W] instance masks are never
 * materialised.  semantic: device float [B,H,W,n_cats+1] (channel n_cats stays 0, as in the reference);
 * goal_cat_host: HOST int32 [B] (-1 = no goal gate) or NULL.  masks may be NULL (the usual case); the other outputs
 * are those of peanut_rcnn_inference.  Synchronises the stream once, as that call does (to read the detection counts). */
int peanut_rcnn_semantic(peanut_rcnn_t* h, const uint8_t* img_bgr, int B, int H, int W, int n_cats, float sem_pred_prob_thr,
                         float goal_thr, const int32_t* goal_cat_host, float* semantic, int* n_det_host, float* boxes,
                         float* scores, int32_t* classes, uint8_t* masks, void* stream);
/* Test / bisect hook: device pointer (and byte capacity) of a stage buffer of the last peanut_rcnn_inference call:
 * "rois" [B*cap,5], "roi_level", "roi_logit", "prop_count" [B], "cls" [B*cap,K+1], "bbox" [B*cap,4K], "det_in" /
 * "det_out" [B,D,4], "det_score", "det_cls", "det_count" [B], "mprobs" [sum n, 2P, 2P], "sel_idx", "sel_score", "nvalid". */
int peanut_rcnn_debug_stage(peanut_rcnn_t* h, const char* name, const void** dev, size_t* bytes);

/* The non-convolution operators of Mask R-CNN inference (detectron2 implements them natively in
 * `detectron2._C` / torchvision: ROIAlign, nms; paste_masks_in_image is a fused resample+threshold).
 * Restated from detectron2 v0.6's published definitions; parity pinned against oracle/rcnn_ref.py only.
 *
 * peanut_roi_align: ROIAlign over up to 4 NHWC pyramid levels in one launch.  feats[l] device [B,h_l,w_l,C],
 * feat_hw = {h_0,w_0,...}, scales[l] = 1/stride_l; rois device [N,5] = (batch, x0, y0, x1, y1) in input pixels,
 * levels device int32 [N]; sampling_ratio 0 = adaptive ceil(roi/pooled); aligned = ROIAlignV2's half-pixel
 * shift; out device [N,pooled,pooled,C]. */
int peanut_roi_align(const float* const* feats, const int* feat_hw, const float* scales, int n_levels, int C,
                     const float* rois, const int* levels, int n_rois, int pooled, int sampling_ratio, int aligned,
                     float* out, void* stream);
/* Greedy NMS of boxes ALREADY sorted by descending score (device [n,4] x0,y0,x1,y1); categories (device
 * int32 [n], may be NULL) restrict suppression to equal ids (= torchvision batched_nms); keep device
 * uint8 [n] (1 = kept); workspace device, peanut_nms_workspace_bytes(n) bytes. */
size_t peanut_nms_workspace_bytes(int n);
int peanut_nms(const float* boxes_sorted, const int* categories, int n, float iou_threshold, void* workspace,
               unsigned char* keep, void* stream);
/* The same for n_segments independent box lists stored back to back (one per image): segment k is
 * boxes_sorted[seg_offsets_host[k] .. seg_offsets_host[k+1]), sorted by descending score inside the segment.
 * workspace >= sum_k peanut_nms_workspace_bytes(n_k) bytes.  One pair of launches per 64 segments. */
int peanut_nms_segments(const float* boxes_sorted, const int* categories, const int* seg_offsets_host, int n_segments,
                        float iou_threshold, void* workspace, unsigned char* keep, void* stream);
/* paste_masks_in_image + threshold: masks device [n,M,M] probabilities, boxes device [n,4] in output-image
 * pixels -> out device uint8 [n,H,W] (1 where the bilinearly resampled mask >= threshold). */
int peanut_paste_masks(const float* masks, const float* boxes, int n, int M, int H, int W, float threshold,
                       unsigned char* out, void* stream);

/* Observation formatting, Agent_Helper._preprocess_obs/_preprocess_depth
 * (nav/agent/agent_helper.py:175-217): per-column invalid-depth fill, >0.99 -> far, metres -> cm
 * (f32(min_d*100.0) + (d*f32(max_d-min_d))*100 -- the two constants are formed in double like the
 * reference's Python floats, min_d / max_d are therefore doubles), then rows/cols ds//2::ds of RGB (the reference's PIL
 * NEAREST resize picks the same pixels), depth and semantics.  rgb [H,W,3] uint8, depth [H,W] fp32 in
 * [0,1] (0 = invalid), sem [H,W,ncat] fp32 -> obs [3+1+ncat, H/ds, W/ds] fp32. */
int peanut_preprocess_obs(const uint8_t* rgb, const float* depth, const float* sem, int H, int W, int ncat, int ds,
                          double min_d, double max_d, float* obs, void* stream);
/* The same (agent_helper.py:175-217) for E frames (1..PEANUT_MAP_MAX_BATCH) in one launch: rgb [E,H,W,3], depth [E,H,W],
 * sem [E,H,W,ncat] -> obs [E, 3+1+ncat, H/ds, W/ds], each frame bit-identical to the single call. */
int peanut_preprocess_obs_batch(const uint8_t* rgb, const float* depth, const float* sem, int E, int H, int W, int ncat, int ds,
                                double min_d, double max_d, float* obs, void* stream);

/* ------------------------------------------------------------------------------------------
 * Stage 1 -- per-instance mask accumulation of SemanticPredMaskRCNN.get_prediction
 * (nav/agent/utils/segmentation.py:47-60): for every detected instance j whose class is in
 * range(n_cats) and whose score passes sem_pred_prob_thr (and goal_thr when class == goal_cat),
 * out[:, :, class] += mask_j.  masks [n,H,W] uint8/bool, classes [n] int32, scores [n] fp32,
 * out [H,W,n_cats+1] fp32 (zeroed by the call; channel n_cats stays zero).  The detector that
 * produces masks/classes/scores is peanut_rcnn_* + peanut_roi_align / peanut_nms / peanut_paste_masks above
 * (or detectron2 itself: the accumulation only needs the three tensors).
 * ---------------------------------------------------------------------------------------- */
int peanut_seg_accumulate(const uint8_t* masks, const int32_t* classes, const float* scores, int n, int H, int W,
                          int n_cats, float sem_pred_prob_thr, float goal_thr, int goal_cat, float* out,
                          void* stream);

/* ------------------------------------------------------------------------------------------
 * Operator-level export: one fused conv (+BN scale/shift, +residual, +ReLU) on NHWC fp32.
 * Mirrors mmcv ConvModule / build_conv_layer+build_norm_layer call sites
 * (prediction/mmseg/models/backbones/resnet.py:164-209, decode_heads/psp_head.py:39-46,86-93).
 * ---------------------------------------------------------------------------------------- */
typedef struct peanut_conv peanut_conv_t;
/* w_oihw_host [cout][cin][kh][kw]; scale/shift host [cout] (NULL -> 1 / 0).  cin_pad = channel
 * count of the NHWC input buffer (multiple of 16, >= cin; extra channels must be zero-weighted,
 * which the packer guarantees).  precision = PEANUT_PREC_*: in the emulated modes a pointwise layer with >= 64 output
 * channels and the position GEMMs of a Winograd layer run on csrc/gemm_rs.hip, every other conv with a multiple of 16 input
 * channels on csrc/conv_rs.hip;
 * peanut_conv_precision() returns the PEANUT_PREC_* mode the layer actually runs in (no silent change of arithmetic).  conv_algo = PEANUT_ALGO_* (AUTO: stride-1 3x3 layers with
 * >= 128 input channels run as Winograd F(4x4,3x3), scratch allocated on first use per shape). */
int peanut_conv_create(peanut_conv_t** out, const float* w_oihw_host, const float* scale_host,
                       const float* shift_host, int cout, int cin, int cin_pad, int kh, int kw, int stride,
                       int pad, int dil, int relu, int precision, int conv_algo);
void peanut_conv_destroy(peanut_conv_t* c);
int peanut_conv_precision(peanut_conv_t* c);
int peanut_conv_set_option(peanut_conv_t* c, const char* key, long long value);
/* x_dev [B,H,W,cin_pad] (or split x_dev [..,c1] ++ x2_dev [..,cin_pad-c1] when x2_dev != NULL),
 * res_dev optional [B,Ho,Wo,cout], y_dev [B,Ho,Wo,cout]. */
int peanut_conv_forward(peanut_conv_t* c, const float* x_dev, const float* x2_dev, int c1, const float* res_dev,
                        float* y_dev, int B, int H, int W, void* stream);

/* ------------------------------------------------------------------------------------------
 * Long-term goal selection: Agent_State.update_global_goal
 * (nav/agent/agent_state.py:376-415) and the geodesic distance transform behind it and behind
 * FMMPlanner.set_goal / set_multi_goal (nav/agent/utils/fmm_planner.py:55-75).  The reference calls scikit-fmm's
 * heap-ordered fast marching on the host (`skfmm.distance`, second order); here the same second-order upwind
 * discretisation is solved by tile-wise relaxation in stages that provably end (csrc/goal.hip; <= 0.14 cell from the
 * heap-ordered march on maze maps, gate 0.5).  scikit-fmm is an absent
 * third-party dependency: parity is pinned against the restatement in oracle/fmm_ref.c only (PARITY UNPINNED).
 * Distances are doubles, in cells.
 * ---------------------------------------------------------------------------------------- */
typedef struct peanut_goal peanut_goal_t;
/* full_h x full_w = the full map (960 x 960); col_rad = args.col_rad, the radius of the dilation disk
 * (skimage.morphology.disk(col_rad), agent_state.py:85).  Allocates ~35 B per cell.  Synchronous. */
int peanut_goal_create(peanut_goal_t** out, int full_h, int full_w, int col_rad);
void peanut_goal_destroy(peanut_goal_t* g);
/* Agent_State.reset (:94-105): forget the last distance weights (`self.dd_wt = None`). */
int peanut_goal_reset(peanut_goal_t* g);
/* relaxation rounds / second-order ordering passes the last solve took (diagnostics) */
int peanut_goal_rounds(peanut_goal_t* g);
int peanut_goal_passes(peanut_goal_t* g);
/* 1 when the last solve's ordering passes reached their fixed point (a pass that changed nothing), 0 when they stopped at
 * the pass cap (6) with the last pass still changing tiles: the field is then the last iterate, not the fixed point. */
int peanut_goal_converged(peanut_goal_t* g);
/* agent_state.py:382-386: trav = ~binary_dilation(rint(full_map[0]), disk(col_rad)); trav[collision_map == 1] = 0;
 * trav[visited_vis == 1] = 1.  full_obstacle device fp32 [H,W]; collision_map / visited_vis device uint8 [H,W] or
 * NULL; trav_out device uint8 [H,W] (NULL: kept inside the handle). */
int peanut_goal_traversible(peanut_goal_t* g, const float* full_obstacle, const uint8_t* collision_map,
                            const uint8_t* visited_vis, uint8_t* trav_out, void* stream);
/* FMMPlanner.set_goal (goal_mask NULL, one goal cell) / set_multi_goal (goal_mask device uint8 [H,W], 1 = goal;
 * pass goal_r = -1): traversible device uint8 [H,W] (0 = masked; goal cells are unmasked like
 * `traversible_ma[goal] = 0` does).  dist_out device double [H,W]; cells that are masked or never reached get
 * +inf (fill_mode 0) or max(reached) + 1 (fill_mode 1 = `ma.filled(dd, np.max(dd) + 1)`, fmm_planner.py:66,74).
 * Synchronises the stream (the solver polls a convergence counter). */
int peanut_fmm_distance(peanut_goal_t* g, const uint8_t* traversible, const uint8_t* goal_mask, int goal_r, int goal_c,
                        int fill_mode, double* dist_out, void* stream);
/* Optional first half of peanut_goal_select, for callers that produce target_pred AFTER the map is final -- in the agent
 * Agent_State.update_state runs update_prediction and then update_global_goal (nav/agent/agent_state.py:240-245), and the geodesic
 * field needs the map, not the prediction.  Call it when full_obstacle, collision_map and visited_vis are complete on `stream`
 * (same arguments as the select that follows): the traversible map, the solver's initialisation and the first batch of relaxation
 * rounds are enqueued on a stream of the handle behind that point of `stream`, without synchronising, so that they run beside
 * whatever the caller enqueues on `stream` next (the prediction forward).  The peanut_goal_select that follows with the same
 * inputs continues there and makes `stream` wait for the field before the weights are formed: results are those of a select
 * alone.  The caller must not write the three map inputs in between.  A select with other inputs, peanut_fmm_distance or
 * peanut_goal_reset lets the begun work run out and ignores it. */
int peanut_goal_select_begin(peanut_goal_t* g, const float* full_obstacle, const uint8_t* collision_map,
                             const uint8_t* visited_vis, const int lmb[4], int loc_r, int loc_c, void* stream);
/* The whole of update_global_goal: traversible map, geodesic field from the agent's cell
 * (clip(loc + lmb[0/2], 0, full - 1)), weights exp(-dd / (dist_weight_temperature / map_resolution)) over the local
 * window lmb = {gx1, gx2, gy1, gy2} with the "sum < 10: keep the last weights" rule, value = target_pred * weights
 * (temperature -1: target_pred alone; 0: frontier mode, exp(-dd'/100) with dd' = inf below 60) and its
 * argmax.  As in the reference, dd is the field after `dd[dd == max(dd)] = inf` (:393): when every cell of the map
 * is reached, the farthest ones weigh 0.  The argmax has np.argmax's semantics (first occurrence; the first NaN wins;
 * always a cell of the window); the sum of the weights is reduced in a fixed order (the same bits on every run).
 * Frontier mode neither uses nor replaces the last weights, and a window of another size forgets them.
 * target_pred device fp32 [gx2-gx1, gy2-gy1].  Outputs (host): goal_rc_out = the argmax
 * cell in local-map coordinates (`np.unravel_index(value.argmax(), value.shape)`); stats_out (optional) =
 * {value max, sum of the fresh weights, 1 if the last weights were kept, relaxation rounds}; dist_out (optional,
 * device double [H,W], +inf = masked / unreachable) and value_out (optional, device double [w,h]) for tests.
 * The "avoid repeating the last goal" bookkeeping (:412-415) is host logic of the caller.  Synchronises. */
int peanut_goal_select(peanut_goal_t* g, const float* full_obstacle, const uint8_t* collision_map,
                       const uint8_t* visited_vis, const int lmb[4], int loc_r, int loc_c, const float* target_pred,
                       double dist_weight_temperature, int map_resolution, int goal_rc_out[2], double stats_out[4],
                       double* dist_out, double* value_out, void* stream);
/* Goal selection for the episodes of a lock-step group (ABI 17): update_global_goal (nav/agent/agent_state.py:376-415) of up to
 * PEANUT_GOAL_MAX_BATCH episodes in the launches and host synchronisations of ONE solve -- a relaxation round of the batch is one
 * launch over (tiles, E), a check is one read-back of the [E][rounds] counters and one synchronisation, the stages between are one
 * launch each.  Every episode keeps its own handle (its field, its last weights, its round hints) and gets, bit for bit, what
 * peanut_goal_select gives on that handle alone: it sees the rounds its own solve would run, with rounds that wake none of its
 * tiles in between (csrc/goal.hip), so an episode may be selected in a batch on one step and alone on the next, in any mix.
 * E = 1 equals the single call.  Refused with PEANUT_EINVAL and nothing enqueued: E outside 1..PEANUT_GOAL_MAX_BATCH, a null or
 * repeated handle, handles that differ in full_h, full_w, col_rad or in the solver options (fmm_blocked, fmm_local32, fmm_inner,
 * fmm_max_passes), local windows of different sizes, bad boundaries, a missing target_pred where the mode needs one.
 * All arrays are HOST arrays of E entries; lmb [E][4] and loc_rc [E][2] as in the single calls; collision_map / visited_vis may be
 * NULL as arrays or per entry. */
#define PEANUT_GOAL_MAX_BATCH 16
/* peanut_goal_select_begin for E handles: traversible maps, initialisation and the first batch of stage-A rounds of all
 * E episodes on a side stream behind this point of `stream`; no synchronisation.  Taken over by the peanut_goal_select_batch that
 * names the same handles in the same order with the same inputs; any other call on one of its handles lets the begun work run
 * out first and then does what it would have done alone. */
int peanut_goal_select_begin_batch(int E, peanut_goal_t* const* g, const float* const* full_obstacle,
                                   const uint8_t* const* collision_map, const uint8_t* const* visited_vis,
                                   const int* lmb, const int* loc_rc, void* stream);
/* peanut_goal_select for E handles.  target_pred: E device pointers (NULL as an array or per entry only with
 * dist_weight_temperature == 0); goal_rc_out host [E][2]; stats_out host [E][4] (optional; [e][3] = the rounds the BATCH enqueued,
 * the same for every e); dist_out / value_out: optional host arrays of E optional device pointers.  peanut_goal_passes /
 * _converged answer per handle from the episode's own counters.  Synchronises, as the single call does (the solver polls its
 * counters; one read-back of all E results at the end). */
int peanut_goal_select_batch(int E, peanut_goal_t* const* g, const float* const* full_obstacle,
                             const uint8_t* const* collision_map, const uint8_t* const* visited_vis,
                             const int* lmb, const int* loc_rc, const float* const* target_pred,
                             double dist_weight_temperature, int map_resolution, int* goal_rc_out, double* stats_out,
                             double* const* dist_out, double* const* value_out, void* stream);

/* ------------------------------------------------------------------------------------------
 * The local planner's short-term goal (ABI 19): Agent_Helper._get_stg (nav/agent/agent_helper.py:374-493) and
 * FMMPlanner.get_short_term_goal (nav/agent/utils/fmm_planner.py:77-116), the heavy part of every agent step.  The reference does
 * it on the host: two scikit-image dilations, a scikit-fmm solve on the (m + 2)^2 padded grid, an 11 x 11 window pick, and up to
 * nine further solves when planning fails.  Here the masks and the pick are three kernels (csrc/stg.hip) around the solver above,
 * which is used as it is; the host reads back one small struct per solve.  scale == 1 only (the agent's value).
 * The scalar state machine around it (collision bookkeeping, action choice, untrap: _plan :228-371) is the caller's.
 * ---------------------------------------------------------------------------------------- */
#define PEANUT_STG_MAX_RAD 16     /* largest dilation radius (collision disk and goal disk) */
#define PEANUT_STG_MAX_STEP 5     /* largest step_size: the (2 step + 1)^2 masks travel in the kernel-argument block */
/* what get_short_term_goal returns, as the window kernel writes it to DEVICE memory */
typedef struct {
  double distance;                /* the field at the agent's cell (subset[du, du]) */
  int32_t stg_r, stg_c;           /* the chosen cell in the coordinates of the field (stg_x + state[0] - du, ...) */
  int32_t stop, replan;           /* distance < 5.0; the window's minimum > -0.0001 */
} peanut_stg_window_t;
/* what _get_stg returns, with how it got there (HOST) */
typedef struct {
  double stg_x, stg_y;            /* local-map cells: the `- 1` of :491 applied (x1 = y1 = 0) */
  double distance;
  int32_t stop, replan;           /* of the last solve */
  int32_t retried;                /* 1: the first solve asked to replan and the eroded map was solved (:443-469); with only_explore
                                   * the caller's next_preset_goal() (:444-445) is due */
  int32_t n_magnify, n_solves;    /* goal dilations of the "make the goal larger" loop (:473-489); solves in all */
  int32_t reserved;
} peanut_stg_result_t;
/* The planner's traversible map (:377-420; erode = 1: the retry's, :448-461).  obstacle: device fp32 [m, m] with `row_stride`
 * elements between rows (local_map[0] may be a view), read in place.  Obstacle bit = rint(v) != 0; then the four border rules as
 * the reference writes them -- lmb = {gx1, gx2, gy1, gy2}: gx2 == full_w sets the last row, gy2 == full_h the last column,
 * gx1 == 0 row 0 and gy1 == 0 ROW 0 again (the reference's `grid[y1] = 1`); erode: one 4-connected erosion of that grid with
 * cells outside it counting as set (scipy's binary_erosion(border_value=1), which scikit-image calls); then
 * ~dilate(grid, disk(col_rad)), cells outside counting as unset; collision == 1 -> 0, then visited == 1 -> 1, both device uint8
 * [full_w, full_h] read at offset (gx1, gy1) (either may be NULL: no override); then the 3 x 3 block around (start_r, start_c) -> 1 with
 * Python's slice semantics: clipped at the far edge, EMPTY along an axis whose start is 0 (`[-1:2]`).  trav_out: device uint8
 * [(m + 2), (m + 2)], the map offset by one cell inside a ring of 1 (add_boundary).  col_rad <= PEANUT_STG_MAX_RAD, m >= 3,
 * 0 <= start < m.  No synchronisation. */
int peanut_stg_traversible(const float* obstacle, long long row_stride, int m, int full_w, int full_h, const int lmb[4], int col_rad,
                           int erode, const uint8_t* collision, const uint8_t* visited, int start_r, int start_c, uint8_t* trav_out,
                           void* stream);
/* The goal cells (:421, 425-435, 481-484): mask_in device uint8, non-zero = goal -- the [m, m] goal map (in_is_padded = 0: a ring
 * of 0 is added, add_boundary(goal, value=0)) or an already padded [(m + 2), (m + 2)] mask (in_is_padded = 1: the magnify loop) --
 * dilated by disk(radius) inside the padded grid, cells outside it unset; the dilation may spill into the ring, as in the
 * reference.  goal_out: device uint8 [(m + 2), (m + 2)] of 0 / 1, not mask_in.  0 <= radius <= PEANUT_STG_MAX_RAD. */
int peanut_stg_goal(const uint8_t* mask_in, int in_is_padded, int m, int radius, uint8_t* goal_out, void* stream);
/* HOST only, touches no device: get_mask / get_dist (fmm_planner.py:8-36) for scale 1 and the fractional parts (sx, sy) of the
 * state, operation by operation in the reference's order with std::pow for `** 2` and `** 0.5` (CPython's float power is libm's
 * pow).  mask_out, dist_out: host double [(2 step_size + 1)^2]. */
int peanut_stg_masks(double sx, double sy, int step_size, double* mask_out, double* dist_out);
/* get_short_term_goal (:77-116) on a device field: field device double [n, n], state = (state_r, state_c) with 0 <= int(state) < n.
 * The (2 step_size + 1)^2 window at int(state), cells beyond the field = n^2 (np.pad), the reference's arithmetic in double and in
 * its order, np.argmin's semantics (first occurrence, the first NaN wins).  One workgroup; the masks are computed on the host
 * (peanut_stg_masks) and passed by value.  result_dev: DEVICE peanut_stg_window_t.  No synchronisation. */
int peanut_stg_window(const double* field, int n, double state_r, double state_c, int step_size, peanut_stg_window_t* result_dev,
                      void* stream);
/* _get_stg whole.  The handle owns the padded masks, the field and a peanut_goal_t of (m + 2) x (m + 2); every solve is
 * peanut_fmm_distance (goal_mask, fill_mode 1) on the two masks, bit for bit. */
typedef struct peanut_stg peanut_stg_t;
int peanut_stg_create(peanut_stg_t** out, int m, int full_w, int full_h, int col_rad, int step_size);
void peanut_stg_destroy(peanut_stg_t* h);
/* First solve with the goal dilated by disk(found_goal == 1 ? radius_found : 2) (radius_found: 8, 6 for a toilet); if it asks to
 * replan, the eroded traversible map and a second solve on the same goal; if found_goal == 1 and distance > magnify_when_hard:
 * while distance > 100 and the step count <= max_magnify (8, 2 for a toilet), the current padded goal dilated by disk(2) and
 * solved again on the current traversible map.  obstacle / collision / visited / lmb / start as peanut_stg_traversible
 * (start_exact = the agent's position in local-map cells, :264-266; the window's state is start_exact + 1); goal_map device uint8
 * [m, m].  result_out: HOST.  trav_out / goal_out / dist_out: optional device taps ([(m + 2)^2] uint8, uint8, double) of the LAST
 * solve's masks and field.  Synchronises (the loop conditions are host decisions on the struct read back).  PEANUT_EINVAL with
 * nothing enqueued and no output touched: a null pointer, m < 2 step_size + 1, lmb not an m x m window inside the full map,
 * start_exact outside [0, m) on either axis (the reference asserts or wraps there), a radius above PEANUT_STG_MAX_RAD, row_stride < m. */
int peanut_stg_plan(peanut_stg_t* h, const float* obstacle, long long row_stride, const uint8_t* goal_map, const uint8_t* collision,
                    const uint8_t* visited, const int lmb[4], const double start_exact[2], int found_goal, int radius_found,
                    double magnify_when_hard, int max_magnify, peanut_stg_result_t* result_out, uint8_t* trav_out, uint8_t* goal_out,
                    double* dist_out, void* stream);
/* The short-term goals of the episodes of a lock-step group (ABI 20): _get_stg of up to PEANUT_STG_MAX_BATCH episodes, each with
 * its own peanut_stg_t, in the launches and host synchronisations of the LONGEST chain among them.  Every episode is the state
 * machine of peanut_stg_plan (first solve, the eroded retry if it asks to replan, the magnify steps) under exactly its conditions;
 * the call runs in waves: every unfinished episode prepares the masks of its next solve (the traversible maps of a wave in one
 * launch, the grown goals in one), one batched solve of the solver above follows (a relaxation round is one launch over
 * (tiles, E), csrc/goal.hip), one window launch over the episodes, one read-back of the [E] window structs and one
 * synchronisation; the host then advances each episode.  The number of waves is the largest n_solves of the batch, not the sum
 * (peanut_stg_waves).  The window masks (start_exact is fixed for the call) go up once per call through a pinned table; nothing is
 * allocated and no stream is made per wave (the tables belong to the first handle, made on its first batch).  Every episode gets,
 * bit for bit, the result struct and the taps peanut_stg_plan gives on its handle alone, whatever the handles were used for
 * before; E = 1 equals peanut_stg_plan.
 * Arguments as a descriptor: `size` = sizeof(peanut_stg_batch_t) first, so that a caller built against another layout is refused.
 * All arrays are HOST arrays of E entries: h the handles; obstacle / goal_map / collision / visited device pointers and row_stride,
 * found_goal, radius_found, magnify_when_hard, max_magnify as the arguments of peanut_stg_plan; lmb [E][4]; start_exact [E][2];
 * result_out [E] (host); trav_out / goal_out / dist_out optional arrays of E optional device taps of each episode's LAST solve.
 * The stream the work is enqueued on travels in the descriptor.  Synchronises (once per wave, and inside every solve).
 * PEANUT_EINVAL with nothing enqueued and no result or tap written: a wrong size, E outside 1..PEANUT_STG_MAX_BATCH, a null array
 * or a null entry (the tap arrays and their entries excepted), the same handle twice, handles that differ in m, full_w, full_h,
 * col_rad, step_size or the solver options, and every per-episode condition peanut_stg_plan refuses.  A solve that fails part-way
 * lets the stream run out before the error returns. */
#define PEANUT_STG_MAX_BATCH PEANUT_GOAL_MAX_BATCH
typedef struct {
  uint64_t size;                          /* sizeof(peanut_stg_batch_t) */
  int32_t E, reserved;
  peanut_stg_t* const* h;
  const float* const* obstacle;
  const long long* row_stride;
  const uint8_t* const* goal_map;
  const uint8_t* const* collision;
  const uint8_t* const* visited;
  const int* lmb;                         /* [E][4] */
  const double* start_exact;              /* [E][2] */
  const int* found_goal;
  const int* radius_found;
  const double* magnify_when_hard;
  const int* max_magnify;
  peanut_stg_result_t* result_out;        /* [E], host */
  uint8_t* const* trav_out;               /* optional */
  uint8_t* const* goal_out;               /* optional */
  double* const* dist_out;                /* optional */
  void* stream;
} peanut_stg_batch_t;
int peanut_stg_plan_batch(const peanut_stg_batch_t* batch);
/* Test hook: the synchronising waves of the last plan this handle took part in (peanut_stg_plan: its n_solves; a batch: the
 * largest n_solves among its episodes). */
int peanut_stg_waves(peanut_stg_t* h);

/* ------------------------------------------------------------------------------------------
 * The planner's map bookkeeping (ABI 22; csrc/plan.hip): what Agent_Helper._plan writes into visited_vis and collision_map on
 * every step (nav/agent/agent_helper.py:272-315) before _get_stg reads them -- the planner-side sibling of
 * peanut_map_mark_agent(_batch).  The scalar state machine of _plan (collision test, action choice, untrap) stays the caller's
 * (peanut_amd.agent_helper.Agent_Helper); the device never sees a float.
 * ---------------------------------------------------------------------------------------- */
#define PEANUT_PLAN_LINE_POINTS 26    /* draw_line's steps + 1 */
#define PEANUT_PLAN_MAX_CELLS 28      /* 4 lengths x 7 widths of the collision loop (:302-303; the reference's width is always 1, :294) */
#define PEANUT_PLAN_MAX_BATCH 16
/* HOST only, touches no device: the points of vu.draw_line(last_start, start, .) (nav/agent/utils/visualization.py:19-24):
 * points_out[i][a] = rint(last_start[a] + (start[a] - last_start[a]) * i / 25) for i = 0..25 -- an integer product, one correctly
 * rounded division, one add, all in double, and rint to nearest-even: IEEE operations only, NumPy's bits. */
int peanut_plan_line(const int last_start[2], const int start[2], int points_out[PEANUT_PLAN_LINE_POINTS][2]);
/* What the calls below share (HOST struct, copied by value): the size of every map and the stream the launch is enqueued on
 * (NULL = default stream).  For a following peanut_stg_plan / peanut_goal_select_begin to see the marks, give them the same
 * stream, or one ordered behind it. */
typedef struct {
  int32_t full_w, full_h;                 /* 2..65536 */
  void* stream;
} peanut_plan_maps_t;
/* One episode's step (HOST struct, copied by value; the maps are DEVICE uint8 [full_w, full_h], contiguous, distinct). */
typedef struct {
  uint8_t* visited_vis;
  uint8_t* collision_map;
  int32_t lmb[4];                         /* gx1, gx2, gy1, gy2: an m x m window inside the full map, 2 <= m <= 4096 */
  int32_t last_start[2];                  /* window cells in [0, m): the last position formed in THIS step's window and thresholded */
  int32_t start[2];                       /* (:267-277) */
  int32_t n_cells;                        /* 0..PEANUT_PLAN_MAX_CELLS */
  int32_t cells_rc[PEANUT_PLAN_MAX_CELLS][2];   /* full-map cells (r, c), already thresholded (:311-314) */
} peanut_plan_mark_t;
/* `visited_vis[gx1:gx2, gy1:gy2] = vu.draw_line(last_start, start, visited_vis[gx1:gx2, gy1:gy2])` (:278-280) and
 * `collision_map[r, c] = 1` for the given cells (:315), in ONE launch: one thread per (line point, corner) and per cell, plain
 * byte stores of 1, nothing read, no atomics.  Every point (x, y) of peanut_plan_line sets mat[x - 1:x + 1, y - 1:y + 1] = 1 with
 * Python's slice semantics on the m x m view: rows x - 1 and x, and NOTHING along an axis whose coordinate is 0 (`[-1:1]` is empty
 * for m >= 2) -- the reference's behaviour, kept.  Enqueued on maps->stream.  No synchronisation, no allocation.
 * PEANUT_EINVAL with nothing enqueued and no map touched: a null pointer, m < 2, lmb not an m x m window inside the full map, a
 * start or last_start outside [0, m), n_cells outside its range, a cell outside the map, an episode whose two maps overlap. */
int peanut_plan_mark(const peanut_plan_maps_t* maps, const peanut_plan_mark_t* episode);
/* The same for the E episodes of a lock-step group in ONE launch (grid (1, E)): episodes HOST [E].  E outside
 * 1..PEANUT_PLAN_MAX_BATCH and two episodes naming the same map are refused as well; one refused episode refuses the whole call
 * and leaves every map as it was.  Every map ends with the bytes E single calls give.  Enqueued on maps->stream.  No
 * synchronisation, no allocation. */
int peanut_plan_mark_batch(const peanut_plan_maps_t* maps, int E, const peanut_plan_mark_t* episodes);

/* ------------------------------------------------------------------------------------------
 * Map datasets on the device (ABI 21; csrc/mapio.hip): the uint8 map sequences nav/collect_maps.py records and
 * prediction/train_prediction_model.py reads, without the fp32 round trip over the host.
 * ---------------------------------------------------------------------------------------- */
#define PEANUT_MAPSEQ_MAX_BATCH 16     /* episodes of one peanut_mapseq_encode */
#define PEANUT_MAPSEQ_MAX_SAMPLES 64   /* samples of one peanut_mapseq_inputs / peanut_mapseq_bce */
/* A snapshot per episode of a lock-step group in one launch (collect_maps.py:81-82: `full_map.cpu().numpy() * 255`,
 * `.astype(np.uint8)`), and the two sums of the dataset filter (:86) from the same pass.  Arguments as a descriptor: `size` =
 * sizeof(peanut_mapseq_encode_t) first, so that a caller built against another layout is refused; the stream the work is enqueued
 * on travels in it.  All arrays are HOST arrays of E entries, copied into the launch by value.  src[e]: device fp32 [C, W, H] read
 * where it lies, plane_stride / row_stride / col_stride in floats (col_stride must be 1); dst[e]: device uint8 [C, W, H],
 * contiguous; dst = (uint8)(src * 255.0f), one fp32 multiply and a truncation -- numpy's bits for every value in [0, 256/255).
 * Outside that range the reference is undefined (a float -> uint8 cast that does not fit); here a negative product and NaN give 0,
 * a product >= 255 gives 255.  sums: DEVICE uint64 [E][2], written whole: [e][0] the sum of the bytes of channels 4:, [e][1] of
 * channel 1 (exact integers).  Rows whose address and length allow it are read with 16-byte loads, chosen per episode from the
 * pointers, strides and H.  No synchronisation.  PEANUT_EINVAL with nothing enqueued: a wrong size, E outside
 * 1..PEANUT_MAPSEQ_MAX_BATCH, C < 5, a null pointer, col_stride != 1, overlapping rows, one dst twice. */
typedef struct {
  uint64_t size;                          /* sizeof(peanut_mapseq_encode_t) */
  int32_t E, C, W, H;
  const float* const* src;
  const long long* plane_stride;
  const long long* row_stride;
  const long long* col_stride;
  uint8_t* const* dst;
  uint64_t* sums;                         /* device [E][2] */
  void* stream;
} peanut_mapseq_encode_t;
int peanut_mapseq_encode(const peanut_mapseq_encode_t* batch);
/* A stored sequence on the device: maps uint8 [T, C, W, H], contiguous; and the stream the calls that read it are enqueued on
 * (NULL = default stream). */
typedef struct {
  const uint8_t* maps;
  int32_t T, C, W, H;
  void* stream;
} peanut_mapseq_t;
/* One sample of it: snapshot t_idx, the S x S window whose first cell is (x1, y1). */
typedef struct {
  int32_t t_idx, x1, y1;
} peanut_mapseq_sample_t;
/* The model inputs of B samples (LoadMapFromFile, train_prediction_model.py:66-68: `maps[t_idx] / 255.` as fp32;
 * peanut_amd.mapio.model_input): out device fp32 [B, C, S, S] = float(byte) / 255.0f, the IEEE division, bit for bit
 * np.float32(k) / np.float32(255) for all 256 bytes.  seq and samples are HOST structs (samples: B of them), copied by value.
 * Enqueued on seq->stream.  No synchronisation.  PEANUT_EINVAL with nothing enqueued: a null pointer, B outside
 * 1..PEANUT_MAPSEQ_MAX_SAMPLES, S outside 1..min(W, H), a t_idx outside [0, T), a window that leaves the map. */
int peanut_mapseq_inputs(const peanut_mapseq_t* seq, const peanut_mapseq_sample_t* samples, int B, int S, float* out);
/* The loss of the reference on B samples (my_loss, train_prediction_model.py:173-184, on the target of :85-89), the target never
 * materialised: logits device fp32 [B, K, S, S] (raw, no sigmoid); the target of cell (k, i, j) of sample b is
 * y = float(maps[T-1, 4+k, x1+i, y1+j] * (maps[t_idx, 1, x1+i, y1+j] == 0)) / 255.0f; the loss of a cell, in double on the promoted
 * x and y, (1 - y) * x + max(-x, 0) + log1p(exp(-|x|)) (binary_cross_entropy_with_logits, reduction 'none').  sum_out: HOST double
 * [B][K], the sum over the window.  The cells are summed over a fixed partition (chunks of 1024 cells, a function of S alone) in a
 * fixed order: the bits of sum_out[b][k] depend on neither B, the sample's slot nor the run.  The logits must be finite.
 * Synchronises seq->stream (the sums come back to the host).  PEANUT_EINVAL with nothing enqueued: as peanut_mapseq_inputs, and K
 * outside 1..C - 4. */
int peanut_mapseq_bce(const peanut_mapseq_t* seq, const peanut_mapseq_sample_t* samples, int B, int S, const float* logits, int K,
                      double* sum_out);
/* Augmented training batches (ABI 25): what the reference's train_pipeline (nav/pred_model_cfg.py:47-56: LoadMapFromFile, Resize
 * at ratio 1, Pad, RandomCrop, RandomFlip, RandomRotate) makes of a sample, input and target, from sequences that stay on the
 * device.  One sample (HOST struct, copied by value): its own sequence maps uint8 [T, C, W, H] (a batch draws from different
 * files; C, W, H are shared), the snapshot t_idx, the crop offsets (off_r, off_c) into the padded map, flip (0 none, 1
 * horizontal = the last axis, 2 vertical = the first map axis), rotate (0 off, else on) and the cosine and sine of the angle,
 * formed by the caller in double. */
typedef struct {
  const uint8_t* maps;
  int32_t T, t_idx, off_r, off_c, flip, rotate;
  double cos_t, sin_t;
} peanut_mapseq_aug_t;
/* The batch: `size` = sizeof(peanut_mapseq_train_t) first; the map is padded with zeros at the bottom and right to
 * (pad_r, pad_c), cropped to (S_r, S_c) at the sample's offsets, flipped, rotated about the centre of the crop.  Per sample and
 * output cell (y, x) of the crop, with cy = (S_r - 1) / 2, cx = (S_c - 1) / 2:
 *   rotation on:  ys = c (y - cy) - s (x - cx) + cy,  xs = s (y - cy) + c (x - cx) + cx   in double
 *                 (mmcv.imrotate with center None and auto_bound False: cv2.getRotationMatrix2D(center, -angle, 1) and
 *                 warpAffine without WARP_INVERSE_MAP)
 *   tap(yi, xi):  0 outside [0, S_r) x [0, S_c) (the constant border; it takes part in the interpolation); else the flip is
 *                 undone (xi <- S_c - 1 - xi for flip 1, yi <- S_r - 1 - yi for flip 2), r = yi + off_r, q = xi + off_c, and the
 *                 tap is 0 where r >= W or q >= H (the padding), else the source cell (r, q)
 *   img  fp32 [B, C, S_r, S_c]: rotation on: the bilinear blend of float(byte) / 255.0f at the taps (floor ys, floor xs),
 *        (., +1), (+1, .), (+1, +1) of snapshot t_idx, the weights (1-fy)(1-fx), (1-fy) fx, fy (1-fx), fy fx formed in double and
 *        rounded to fp32, summed in fp32 in that order; rotation off: float(byte) / 255.0f of tap(y, x), the bits of
 *        peanut_mapseq_inputs
 *   gt   uint8 [B, K, S_r, S_c] (may be NULL: not written): at the nearest tap (floor(ys + 0.5), floor(xs + 0.5)), or (y, x)
 *        with rotation off: maps[T-1, 4+k, r, q] where maps[t_idx, 1, r, q] == 0, else 0 (train_prediction_model.py:85-89; the
 *        explored mask is read at the source cell: the reference masks before it augments).
 * Unpinned (cv2 is absent where the fixtures are made): cv2 quantises warpAffine's source coordinates to 1/1024 px and the
 * bilinear fraction to 1/32 px; the rule here is exact in double and held to a float64 restatement and to scipy's
 * affine_transform(mode='grid-constant').  Resize at ratio 1, Pad, RandomCrop, RandomFlip and the order of the random draws are
 * pinned by the reference's own code.
 * ONE launch for the batch on `stream`: a workgroup owns a 16 x 64 tile of a sample's crop, a thread four consecutive cells of a
 * row.  Every element of img and gt is written.  No synchronisation, no allocation.  PEANUT_EINVAL with nothing enqueued: a wrong
 * size, a null pointer (gt excepted), B outside 1..PEANUT_MAPSEQ_MAX_SAMPLES, C < 5, K outside 1..C - 4, a pad smaller than the
 * map, a crop larger than the pad, an offset outside [0, pad - S], a t_idx outside [0, T), flip outside 0..2, a non-finite cos_t /
 * sin_t or cos_t^2 + sin_t^2 not within 1e-9 of 1. */
typedef struct {
  uint64_t size;                          /* sizeof(peanut_mapseq_train_t) */
  int32_t B, C, W, H;
  int32_t pad_r, pad_c, S_r, S_c;
  int32_t K, reserved;
  const peanut_mapseq_aug_t* samples;     /* HOST [B] */
  float* img;                             /* device [B, C, S_r, S_c] */
  uint8_t* gt;                            /* device [B, K, S_r, S_c], or NULL */
  void* stream;
} peanut_mapseq_train_t;
int peanut_mapseq_train_batch(const peanut_mapseq_train_t* batch);
/* The loss of peanut_mapseq_bce against a GIVEN target (the gt of peanut_mapseq_train_batch): logits device fp32
 * [B, K, S_r, S_c], gt device uint8 of that shape, y = float(byte) / 255.0f; the same cell formula, the same partition (chunks
 * of 1024 cells of the row-major window) and the same fixed order, so that a target equal to the one peanut_mapseq_bce derives
 * gives its bits.  sum_out: HOST double [B][K].  `size` = sizeof(peanut_mapseq_bce_dense_t) first.  Synchronises `stream` (the
 * sums come back to the host).  PEANUT_EINVAL with nothing enqueued: a wrong size, a null pointer, B outside
 * 1..PEANUT_MAPSEQ_MAX_SAMPLES, K, S_r or S_c below 1, a window of 2^31 cells or more. */
typedef struct {
  uint64_t size;                          /* sizeof(peanut_mapseq_bce_dense_t) */
  int32_t B, K, S_r, S_c;
  const float* logits;
  const uint8_t* gt;
  double* sum_out;                        /* HOST [B][K] */
  void* stream;
} peanut_mapseq_bce_dense_t;
int peanut_mapseq_bce_dense(const peanut_mapseq_bce_dense_t* batch);

/* ------------------------------------------------------------------------------------------
 * The agent's visualisation frame (ABI 23; csrc/vis.hip): what Agent_Helper._visualize (nav/agent/agent_helper.py:496-621) builds on
 * the host with PIL, matplotlib, cv2 and scikit-image from maps that live on the device here.  Three launches for 1..16 episodes:
 * the index map, the ranges of the three fields, the frame.  Nothing synchronises, nothing is allocated.
 * Unpinned (cv2 is absent where the fixtures are made): the arrow's fill rule and the nearest resize at inexact ratios follow the
 * rules stated below, not cv2's code; titles are the caller's (they are part of the background image).
 * ---------------------------------------------------------------------------------------- */
#define PEANUT_VIS_H 600
#define PEANUT_VIS_W 1415                  /* init_vis_image: 1165 + 250 (nav/agent/utils/visualization.py:28) */
#define PEANUT_VIS_FRAME_BYTES 2547000     /* 600 * 1415 * 3: a multiple of 8 */
#define PEANUT_VIS_MAX_BATCH 16
#define PEANUT_VIS_RANGE_WORDS 8           /* uint64 words of range workspace per episode */
/* What the episodes of one call share (HOST struct, copied by value). */
typedef struct {
  int32_t m;                     /* the local window is m x m, 1..4096 */
  int32_t channels;              /* planes of local_map = 4 + num_sem_categories, >= 5 */
  int32_t full_w, full_h;        /* collision_map / visited_vis are uint8 [full_w, full_h], contiguous */
  const uint8_t* background;     /* device uint8 [600, 1415, 3] BGR: init_vis_image (visualization.py:27-83) */
  const uint8_t* palette;        /* device uint8 [256][3] RGB: int(x * 255.) of the colour palette, zero beyond it (:545-550) */
  const uint8_t* cmap;           /* device uint8 [257][3] BGR: (cm(i)[[2, 1, 0]] * 255).astype(uint8) of 'Purples', entry 256 the
                                    "bad" colour (:562-567) */
  void* stream;
} peanut_vis_common_t;
/* One episode (HOST struct, copied by value; every pointer a DEVICE pointer). */
typedef struct {
  const float* local_map;        /* fp32, `channels` planes of m x m read where they lie (as peanut_goal_map: strides in elements, */
  long long plane_stride;        /*  column stride 1, planes and rows must not overlap) */
  long long row_stride;
  const uint8_t* collision_map;  /* read at lmb (:519) */
  const uint8_t* visited_vis;    /* (:526) */
  int32_t lmb[4];                /* gx1, gx2, gy1, gy2: an m x m window inside the full map */
  const uint8_t* goal;           /* uint8 [m, m], contiguous: the planner's goal map, non-zero = goal (:538-543) */
  int32_t stg[2];                /* int(self.stg[0]), int(self.stg[1]) (:520-521): marked when both lie below m; a negative
                                    coordinate in [-m, -1] wraps as NumPy's does; below -m the call is refused */
  const uint8_t* rgb;            /* uint8 [480, 640, 3] RGB (self.rgb_vis, :556), or NULL: the background stays */
  const void* target_pred;       /* [m, m] contiguous, or NULL: no overlay, no right panel (:564) */
  const void* value;             /* [m, m] contiguous (:575); needed with target_pred */
  const void* dd_wt;             /* [m, m] contiguous (:582); needed with target_pred */
  int32_t bits[3];               /* 32 (float) or 64 (double) for target_pred, value, dd_wt: the arithmetic of the normalisation */
  int32_t data_bits[3];          /* 32 or 64: what the field is stored as; fp32 data may be normalised in double (the reference's
                                    float64 `temp` filled with fp32 predictions, agent_state.py:362), not the reverse */
  int32_t arrow[4][2];           /* (x, y) frame pixels of get_contour_points (visualization.py:5-16), formed by the caller */
  uint8_t arrow_bgr[4];          /* the colour of :605-607 (b, g, r, unused) */
  uint8_t* index_map;            /* out, uint8 [m, m] */
  uint64_t* ranges;              /* workspace, PEANUT_VIS_RANGE_WORDS words, 8-byte aligned; needs no initialisation */
  uint8_t* frame;                /* out, uint8 [600, 1415, 3] BGR, 8-byte aligned (peanut_vis_index_map: unused) */
} peanut_vis_episode_t;
/* The index map alone, ONE launch (:512-543 and agent_state.py:259-262).  Per cell of the window:
 *   sem = argmax_c local_map[4 + c], the last plane taken as 1e-5f, the first maximum winning (NaN ranks highest, as torch.argmax)
 *   sem += 5; a collision cell -> 14; the cell stg -> 15
 *   no_cat = sem == num_sem_categories + 4:  -> 0; and rint(exp) == 1 -> 2; and rint(obstacle) == 1 -> 1      (in this order)
 *   visited -> 3; within the disk(4) dilation of goal (cells outside the map unset) -> 4.
 * With num_sem_categories == 10 the value 14 IS the no-category value, so collision cells fall under those rules: the
 * reference's behaviour, kept.  Also initialises episode->ranges.  PEANUT_EINVAL with nothing enqueued: a null pointer (rgb and
 * the three fields may be NULL), m or channels outside their ranges, overlapping strides, lmb not an m x m window inside the full
 * map, a stg coordinate below -m. */
int peanut_vis_index_map(const peanut_vis_common_t* common, const peanut_vis_episode_t* episode);
/* The frame, THREE launches on common->stream:
 *   1. the index map as above;
 *   2. the NaN-propagating minimum and maximum of target_pred, value and dd_wt (np.min / np.max: exact, so independent of the
 *      order of reduction), skipped without a target_pred;
 *   3. the frame, every thread forming 8 consecutive bytes and storing them as two words:
 *      the background; rgb flipped to BGR at [50:530, 15:655]; at [50:530, 670:1150] the index map through the palette, flipped
 *      upside down, BGR, resized to 480 x 480 (:545-557), and where that colour is pure white (b + g + r == 765) and a prediction
 *      exists the colour of target_pred (:565-572); with a prediction dd_wt at [50:290, 1165:1405], value at [290:530, 1165:1405]
 *      (240 x 240) and the grey (100) borders of :589-592; the arrow over all of it.
 *   colour of a field value x: normed = (x - min) / (max - min) in the field's own arithmetic (float or double);
 *      idx = (int)(normed * 256), 255 where normed == 1; NaN (max == min, or a NaN in the field) -> entry 256.
 *   resize (cv2's INTER_NEAREST): src = min((int)floor(dst * ifx), n - 1), ifx = 1.0 / ((double)dst_n / src_n), in double.
 *   arrow: a pixel is painted iff its integer centre lies in the closed polygon of the four vertices -- inside by crossing
 *      number (even-odd) or on an edge -- in integer arithmetic, clipped to the frame.
 * PEANUT_EINVAL with nothing enqueued: as peanut_vis_index_map; a target_pred without value or dd_wt; bits or data_bits other than 32 / 64, or bits below data_bits; a
 * frame or ranges pointer that is not 8-byte aligned; an arrow vertex outside +-2^20. */
int peanut_vis_render(const peanut_vis_common_t* common, const peanut_vis_episode_t* episode);
/* The same for E episodes (1..PEANUT_VIS_MAX_BATCH) of one map size in the same three launches (the episode is a grid dimension):
 * episodes HOST [E]; frame e has the bits of the single call.  Two episodes naming the same frame, index_map or ranges are
 * refused; one refused episode refuses the whole call and nothing is enqueued. */
int peanut_vis_render_batch(const peanut_vis_common_t* common, int E, const peanut_vis_episode_t* episodes);
/* The arg-max of the semantic planes alone (agent_state.py:259-262: `vlm = local_map[4:]; vlm[-1] = 1e-5; vlm.argmax(0)`): out
 * device uint8 [m, m] in one launch on common->stream; of `common` only m, channels and stream are read; local_map as above.
 * No synchronisation.  PEANUT_EINVAL: a null pointer, bad dimensions or strides. */
int peanut_vis_sem_argmax(const peanut_vis_common_t* common, const float* local_map, long long plane_stride, long long row_stride,
                          uint8_t* out);
/* Device views into a goal handle (peanut_goal_select's `self.dd_wt` and `self.value`, agent_state.py:409-410): *dd_wt_out and
 * *value_out point at double [lw, lh] of the last select (value only if that select was given no value_out of its own); dims_out
 * = {lw, lh}.  No copy, no launch; valid until the next select on the handle.  PEANUT_EINVAL: a null argument, no select yet. */
int peanut_goal_fields(peanut_goal_t* h, const double** dd_wt_out, const double** value_out, int dims_out[2]);

/* ------------------------------------------------------------------------------------------
 * Multi-GPU: collation of the predicted maps for logging.  One process per GPU, maps /
 * episodes sharded with no data-path collective -- the reference shards by hand with --start_ep/--end_ep/
 * --sem_gpu_id (nav/arguments.py:15-20, nav/collect.py:37-50) and never communicates; this all-gather is the one
 * collective BASELINE.json's north_star adds.  RCCL over xGMI, bound at run time (the librccl.so already loaded
 * in the process, e.g. torch's, else ROCm's; PEANUT_RCCL_LIB overrides).
 * ---------------------------------------------------------------------------------------- */
#define PEANUT_COMM_ID_BYTES 128
typedef struct peanut_comm peanut_comm_t;
/* rank 0: create the id (ncclGetUniqueId), then hand the 128 bytes to every rank (host side: file, MPI, TCP store). */
int peanut_comm_unique_id(unsigned char id[PEANUT_COMM_ID_BYTES]);
/* every rank, on its own GPU (the current HIP device): ncclCommInitRank -- a collective call.  n_ranks == 1 needs
 * neither an id nor RCCL. */
int peanut_comm_create(peanut_comm_t** out, int n_ranks, int rank, const unsigned char id[PEANUT_COMM_ID_BYTES]);
void peanut_comm_destroy(peanut_comm_t* c);
int peanut_comm_info(peanut_comm_t* c, int* n_ranks, int* rank);
/* which RCCL library got bound ("" when none could be) */
const char* peanut_comm_backend(void);
/* local: this rank's [B_local,K,S,S] fp32 maps (device, `count` floats); all: [n_ranks * count] floats (device),
 * rank-major.  One ncclAllGather on `stream`, no staging copy, no synchronisation. */
int peanut_allgather_maps(peanut_comm_t* c, const float* local, float* all, size_t count, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PEANUT_HIP_H_ */
