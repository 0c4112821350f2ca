/*
 * r50.h — C ABI of libr50hip.so: MI355X (gfx950) ResNet-50 feature extraction.
 *
 * The reference (ferreiraluisa/implementation-phd-lab-vision) has no FFI/plugin registry; its
 * boundary for this path is a Python call on an nn.Module-like object:
 *
 *     backbone = nn.Sequential(*list(resnet50(...).children())[:-1]).to(device).eval()
 *                                          -- src/preprocess_resnet_features.py:207-209
 *     feats = backbone(x).flatten(1)       -- src/preprocess_resnet_features.py:242,296
 *
 * Each entry point below cites the reference interface it replaces.  Plain pointers and sizes
 * only: no torch types, no exceptions across the boundary.  Every function returns 0 on success
 * or a negative r50_status; r50_last_error() gives the text.  One handle per (device, stream);
 * a handle is not re-entrant.  All device pointers are owned by the caller (e.g. PyTorch
 * allocations); the handle owns its packed weights and activation workspace.
 *
 * Layouts:  frames   fp32 NCHW (n,3,224,224), ImageNet-normalised, contiguous
 *                    (what src/dataset.py:242-245,429 produces and :295 reshapes)
 *           features fp32 (n,2048) row-major (= backbone(x).flatten(1), :296)
 *           internal activations bf16 NHWC.
 *
 * Pointer alignment ("Pointer alignment").  Every DEVICE pointer of this ABI (r50.h and the r50_*.h family headers)
 * has a required alignment in bytes:
 *   - R50_ALIGNED(n) in front of the parameter's name: the address must be a multiple of n.  n is the widest access the kernels make
 *     through that pointer (a 16-byte buffer or vector load, a packed 4-byte store, ...); where a kernel reads p + row * pitch with such an
 *     access, the entry point's size checks (cin, c, d, cpad, ld multiples) make every row start a multiple of n as well.
 *   - every `void*` / `const void*` device pointer carries one: it has no natural alignment, its element type depends on the op or on `et`.
 *   - a typed pointer (float*, double*, int*, int64_t*) without one needs the natural alignment of its type, and the op works at every
 *     such address.
 * Every entry point checks its annotated pointers after the null checks and before its first launch, copy or attribute call: a pointer
 * below its alignment returns R50_ERR_INVALID, r50_last_error() names the parameter and the bytes, and nothing was touched.  NULL, where
 * NULL is allowed, counts as aligned.  A contiguous slice of a larger tensor is therefore a legal operand down to the stated alignment.
 * HOST pointers (named *_host, descriptors, out-parameters such as dims_out) need only their type's natural alignment; `stream` and
 * handles are not operands.  tests/test_alignment_gpu.py runs every op with every operand at exactly an odd multiple of its requirement.
 */
#ifndef R50_H_
#define R50_H_

#include <stddef.h>
#include <stdint.h>

#ifndef R50_ALIGNED
#define R50_ALIGNED(n)      /* read by people and by tests/alignment.py: the device pointer that follows must be a multiple of n bytes */
#endif

#ifdef __cplusplus
extern "C" {
#endif

typedef struct r50_handle r50_handle;

typedef enum r50_status {
    R50_OK = 0,
    R50_ERR_INVALID = -1,   /* bad argument (null pointer, n out of range, unknown name ...) */
    R50_ERR_HIP = -2,       /* a HIP runtime call failed */
    R50_ERR_STATE = -3,     /* e.g. forward before weights were loaded */
    R50_ERR_NOMEM = -4
} r50_status;

typedef enum r50_precision {
    R50_PREC_BF16 = 1,      /* bf16 operands, fp32 MFMA accumulation (the reference's CUDA autocast
                               dtype, src/preprocess_resnet_features.py:290-294) */
    R50_PREC_FP32X = 2,     /* fp32-class accuracy on the bf16 matrix cores: every value travels as a bf16
                               (head, tail) pair, each conv is three bf16 MFMA products with fp32 accumulation
                               (the reference's CPU numerics, autocast disabled, :239-241; ~3x the bf16 cost) */
    R50_PREC_BF16W2 = 3,    /* bf16 activations, every bottleneck conv weight as a (head, tail) pair of bf16: two MFMA
                               products per conv, one fp32 accumulator, activation traffic as in bf16 mode.  The bf16
                               error of this network is dominated by WEIGHT rounding, so this is enough to bring the
                               features within 1e-3 (rel-L2) of the fp32 reference at about half the fp32x cost */
    R50_PREC_FP16 = 4,      /* IEEE half operands and activations, fp32 MFMA accumulation: the bf16 path with the other
                               16-bit format (same kernels, same traffic, same speed; conversions saturate at 65504).
                               11 significand bits instead of 8 put the features 3e-4 from the fp32 reference */
    R50_PREC_FP8 = 5        /* BASELINE configs[4]: stem + layer1 as in bf16 mode (their 64-channel convs cannot fill a
                               128-byte fp8 K row), layer2-4 with OCP e4m3 weights and activations on the K = 128 scaled fp8
                               MFMA (per-tensor scales, fp32 accumulation).  Needs r50_set_fp8_scales before the first
                               forward.  A throughput mode: the features are ~1e-1 (rel-L2) from the fp32 reference */
} r50_precision;

/* One host tensor handed to r50_load_weights: torchvision state-dict key + fp32 data. */
typedef struct r50_tensor_desc {
    const char* name;       /* e.g. "layer1.0.conv1.weight", "bn1.running_var" */
    const float* data;      /* host pointer, contiguous fp32 (conv weights OIHW) */
    int64_t numel;
} r50_tensor_desc;

/* Replaces: backbone construction + .to(device) (preprocess_resnet_features.py:207-209).
 * Allocates workspace for batches of up to max_batch frames on HIP device `device_id`. */
int r50_create(r50_handle** out, int device_id, int precision, int max_batch);

/* Replaces: resnet50(weights=IMAGENET1K_V2) state loading + .eval() (:207-209).
 * Takes every conv weight and BN weight/bias/running_mean/running_var by torchvision key name
 * (fc.* and num_batches_tracked are not needed), folds eval-mode BN (eps 1e-5) into conv
 * weight+bias in fp32, converts to bf16 and uploads in the kernels' packed layout.
 * The caller keeps ownership of the host buffers.  R50_ERR_STATE for a handle that takes part in r50_share_weights (a sharer, or an
 * owner that still has sharers): its buffers are read by other handles' launches -- load into a fresh handle instead. */
int r50_load_weights(r50_handle* h, const r50_tensor_desc* tensors, int n_tensors);

/* Instead of r50_load_weights: `h` (fresh from r50_create, same device and precision as `from`, bf16 or fp16) reads the folded / packed weight buffers
 * of `from` -- a second backbone copy for a second batch in flight (backbone.BackboneLanes) without a second copy of the 47 MB of weights.  `h` keeps
 * its own activation workspace, streams, options and profile.  Either handle may be destroyed first: the buffers go with the last one. */
int r50_share_weights(r50_handle* h, r50_handle* from);

/* Replaces: backbone(x).flatten(1) (:242,296).  Asynchronous on `stream` (a hipStream_t; NULL =
 * default stream).  x_nchw_f32_dev: (n,3,224,224) fp32 on the device; out_f32_dev: (n,2048).
 * n may exceed max_batch: the call then loops over chunks of max_batch frames.  x is R50_ALIGNED(16) (r50_forward_u8: 4): the fused stem
 * loads 4 pixels at a time; out is R50_ALIGNED(16): the average pool stores f32x4. */
int r50_forward(r50_handle* h, const float* R50_ALIGNED(16) x_nchw_f32_dev, int n, float* R50_ALIGNED(16) out_f32_dev, void* stream);

/* Same path, one step further upstream: frames as the resized uint8 crops the reference
 * holds right before `frames.to(torch.float32) / 255.0` (src/dataset.py:141-150) and `Normalize(mean, std)`
 * (:242-245), i.e. uint8 NCHW (n,3,224,224).  The three fp32 operations ((u8/255) - mean[c]) / std[c] are done
 * in the stem kernel, bit-identical to the host path; the boundary moves 150,528 B per frame instead of 602,112. */
int r50_forward_u8(r50_handle* h, const uint8_t* R50_ALIGNED(4) x_nchw_u8_dev, int n, float* R50_ALIGNED(16) out_f32_dev, void* stream);

/* Debug hook for per-layer parity tests (no reference counterpart; equivalent to a forward hook
 * on the nn.Sequential).  Runs the network on x (n <= max_batch) and copies the named bf16 NHWC
 * activation into out_bf16_nhwc_dev.  Names: "stem", "pool", "layer{1..4}.{b}",
 * "layer{i}.{b}.t1", ".t2", ".ds".  dims_out receives {N,H,W,C}. */
int r50_forward_layer(r50_handle* h, const float* R50_ALIGNED(16) x_nchw_f32_dev, int n, const char* layer,
                      void* R50_ALIGNED(2) out_bf16_nhwc_dev, int64_t out_capacity_bytes, int64_t dims_out[4],
                      void* stream);

/* Options: "micro_batch" (frames per pass through the layer stack, 0 = whole batch),
 * "profile" (1 = bracket every kernel launch with HIP events, see r50_profile_*),
 * "streams" (1..4: split the batch over internal streams forked from / joined to the caller's; default 1),
 * "overlap_ds" (1 = downsample convs on a side stream; default 0), "fused_stem" (default 1),
 * "fuse_tail" (layer1 / layer2: conv3 + identity + ReLU + the next block's conv1 in one kernel; default 1),
 * "fuse_tail3" (layer3.1-.4: the same pair chained through LDS in one launch; default 1; needs "fuse_tail"),
 * "fuse_block1" (layer1: the same for the 56x56 body, bneck_block1_kernel; 1 = layer1.1, 2 = layer1.2 as well, 3 = layer1.0 too, with its
 * downsample conv computed in the kernel; default 3; needs "fuse_tail"; same bits),
 * "fuse_tail3_last" (layer3.5, whose next conv1 does not fit the chain: conv3 + identity + ReLU alone through the pipelined tail kernel; default 1;
 * same bits),
 * "fuse_cat_chain" (layer2.0: conv3 + downsample + ReLU as one two-source conv chained with layer2.1.conv1 in one launch,
 * bneck_catchain_kernel; default 1; same bits),
 * "sub_out" (layer1.2 stores only the even rows and columns of its output, the ones layer2.0's stride-2 downsample conv reads -- layer2.0.conv1
 * is computed in the same launch; default 1; needs "fuse_block1" >= 2 and "fuse_cat_chain"; same features; debug taps always see full tensors),
 * "fuse_block2" (layer2.1-.3: conv2 + conv3 + identity + ReLU [+ the next conv1] in one launch, t2 kept in LDS; default 1; needs
 * "fuse_tail"; same bits),
 * "fuse_fp8_handover" (R50_PREC_FP8: layer1's output quantised to e4m3 in layer1.2.conv3's epilogue instead of in a pass of its
 * own; default 1; same bits either way),
 * "tile" (force an igemm tile id for every conv, 0 = tuned table; also turns "fuse_tail" off),
 * measurement knobs, all results bit-identical: "inplace_out" (1 = plain-identity blocks write their output over their input;
 * default 0), and PROCESS-WIDE ones (they apply to every handle of the process): "cu_cap" (workgroups a persistent launch may use,
 * 0 = every CU; for pipelines that share the chip; tests/test_work_distribution_gpu.py holds every persistent kernel and the whole network to
 * the uncapped bits under caps of 1 .. 100 workgroups), "tail3_bp" (real pixels per tile of the chained layer3 tail, 0 = automatic), "use_g8" (the
 * eight-phase GEMM tiles of gemm8p_kernel for the streaming 1x1 convs: 0 = never, 1 = on the shapes where they measured faster, the default,
 * 2 / 3 = wherever the shape fits, 256 / 224 pixels per tile), "use_s2" (0 = generic tiles for the stride-2 3x3 shapes) and "stem_strip"
 * (pooled-row pairs per strip of the fused stem kernel, 0 = chosen from the batch). */
int r50_set_option(r50_handle* h, const char* key, int64_t value);
int r50_get_option(r50_handle* h, const char* key, int64_t* value);

/* Per-kernel timing from HIP events recorded on the launch stream while option "profile" is 1.
 * r50_profile_collect synchronises the recorded events and accumulates them; then
 * r50_profile_count / r50_profile_entry enumerate kernel classes ("igemm", "conv1", "maxpool",
 * "avgpool", "stem_pack") and then one entry per bottleneck conv (named by its torchvision key, e.g.
 * "layer3.4.conv2"; "conv1" stays in its class), with launch count, total ms, algorithmic flops and bytes. */
int r50_profile_reset(r50_handle* h);
int r50_profile_collect(r50_handle* h);
int r50_profile_count(r50_handle* h);
int r50_profile_entry(r50_handle* h, int i, const char** name, int64_t* launches, double* total_ms,
                      double* flops, double* bytes);

/* Debug hook: copy the folded+packed parameters of one conv back to the host (BN-fold parity
 * tests).  conv_key e.g. "layer2.0.downsample.0"; what: 0 = bf16 weights in (cout,k,k,cin) order
 * (stem: the kernel's [kh][row][8][4] image), 1 = fp32 folded bias.
 * Bytes of what = 0 for a bottleneck conv, by precision: bf16 / fp16 cout*k*k*cin*2; R50_PREC_BF16W2 twice that, rows
 * (cout,k,k,[w_head(cin) | w_tail(cin)]); R50_PREC_FP32X three times, rows (cout,k,k,[w_head | w_head | w_tail]); R50_PREC_FP8 from layer2
 * on cout*k*k*cin (one e4m3 byte per weight).  "conv1" (the stem): 7*64*64 bytes in every precision -- in R50_PREC_FP32X that is the
 * head image only, the tail image is not served. */
int r50_get_packed(r50_handle* h, const char* conv_key, int what, void* dst_host, int64_t capacity_bytes,
                   int64_t* bytes_out);

/* R50_PREC_FP8 only: per-tensor activation scales (real value = stored fp8 value x scale) of the fp8 part, in execution order:
 * scales[0] = layer1's output (the bf16 -> fp8 hand-over), then per bottleneck of layer2, layer3, layer4: conv1 output, conv2 output,
 * [downsample output, first block of a layer only], block output: R50_FP8_NUM_SCALES values (calibrated on the host, e.g. 1.25 x
 * absmax / 448 of the bf16 network's tensors: backbone.py).  Weight scales are chosen by r50_load_weights (absmax / 448 per conv). */
#define R50_FP8_NUM_SCALES 43
int r50_set_fp8_scales(r50_handle* h, const float* scales, int n);
const char* r50_last_error(r50_handle* h);   /* h may be NULL: last error of r50_create / r50_op_* */
void r50_destroy(r50_handle* h);             /* replaces: del backbone */
const char* r50_version(void);

/* ---- Op-level entry points (per-kernel parity tests; each mirrors one nn.Module of the
 * reference's Sequential, upstream torchvision models/resnet.py).  bf16 NHWC device buffers.
 * Alignment of the convolution, bottleneck, stem and pool hooks: every tensor, weight and bias pointer is R50_ALIGNED(16).  The loaders
 * move 16 bytes per lane through buffer descriptors built on x, w, residual and y (LDS-direct loads included), the shape-specialised
 * and fused kernels read w / w1 / w3 / wd as 16-byte vectors, and the epilogues read the bias as f32x4; the channel checks (cin, cout
 * multiples of 64, 128 for fp8; c % 8 for the pools) make every pixel row a multiple of 16 bytes as well.
 * Size limits ("Size limits").  The matrix-core kernels address every activation tensor through a buffer descriptor and
 * 32-bit byte offsets, and mark a padded tap with the offset 2^31, which the descriptor's range check turns into zeros: a tensor's bytes
 * (for x plus the reach of a padded tap behind its last pixel) must stay BELOW 2^31.  Each entry point states its limits in terms of its
 * arguments ("Size limits:" in its comment; products are exact integers, ho / wo the output height / width).  One step beyond a limit
 * returns R50_ERR_INVALID before anything is queued on the stream, r50_last_error() names the op, the quantity with its value, and the
 * bound, and no operand was touched.  tests/test_size_limits_gpu.py runs every entry point exactly at its limit and one image beyond. ---- */

/* conv2d(k x k, stride, pad, bias=folded BN) [+ residual] [+ ReLU].  w_ohwi_bf16: (cout,k,k,cin)
 * bf16; bias fp32 (cout); residual/y: (n,ho,wo,cout) bf16.  cin % 64 == 0, cout % 64 == 0,
 * k in {1,3}.  tile: 0 = auto, else a tile-config id.
 * Size limits: n*ho*wo <= 2^30; n*h*w*cin*2 + (pad*w+pad)*cin*2 < 2^31 (x bytes, plus what a padded tap reaches behind them);
 * n*ho*wo*cout*2 < 2^31 (y, and the residual); cout*k*k*cin*2 < 2^31 (w).  The same for every tile id.  */
int r50_op_conv2d(const void* R50_ALIGNED(16) x_nhwc_bf16, int n, int h, int w, int cin, const void* R50_ALIGNED(16) w_ohwi_bf16,
                  const float* R50_ALIGNED(16) bias_f32, const void* R50_ALIGNED(16) residual_nhwc_bf16, void* R50_ALIGNED(16) y_nhwc_bf16,
                  int cout, int ksize, int stride, int pad, int relu, int tile, void* stream);
/* The same with IEEE-half tensors (R50_PREC_FP16's element type).  Size limits: those of r50_op_conv2d, term for term (n*ho*wo <= 2^30, and
 * below 2^31: n*h*w*cin*2 + (pad*w+pad)*cin*2, n*ho*wo*cout*2, cout*k*k*cin*2). */
int r50_op_conv2d_f16(const void* R50_ALIGNED(16) x_nhwc_f16, int n, int h, int w, int cin, const void* R50_ALIGNED(16) w_ohwi_f16,
                  const float* R50_ALIGNED(16) bias_f32, const void* R50_ALIGNED(16) residual_nhwc_f16, void* R50_ALIGNED(16) y_nhwc_f16,
                  int cout, int ksize, int stride, int pad, int relu, int tile, void* stream);

/* The two (head, tail) pair precisions at kernel level (debug hooks for per-kernel parity tests): the conv launches of R50_PREC_BF16W2 and
 * R50_PREC_FP32X with caller-owned buffers, built and launched exactly as the network's own convs are.  bf16 only; head = bf16(v),
 * tail = bf16(v - head).  Arguments are checked as in r50_op_conv2d.
 *  r50_op_conv2d_w2: x (n,h,w,cin) bf16; w_pair (cout,k,k,2*cin) = [w_head(cin) | w_tail(cin)] per tap, the packed layout of bf16w2
 *    mode; bias, residual, y and `tile` as in r50_op_conv2d: y = bf16(act(x . w_head + x . w_tail + bias [+ residual])), one fp32
 *    accumulator.  Only the generic, persistent and role-specialised tile ids read a weight pair: the shape-specialised ids (80, 81, 82,
 *    83, 84) are refused with R50_ERR_INVALID before any launch.
 *  r50_op_conv2d_split: x_pair (n,h,w,2*cin) = [head(cin) | tail(cin)] per pixel; w_trip (cout,k,k,3*cin) = [w_head | w_head | w_tail]
 *    per tap, the packed layout of fp32x mode; residual_pair / y_pair (n,ho,wo,2*cout) = [head(cout) | tail(cout)] per pixel:
 *    v = act(x_head . w_head + x_tail . w_head + x_head . w_tail + bias [+ r_head + r_tail]) in fp32, stored as the pair of v.  No tile
 *    argument: 64 couts x 128 pixels when cout % 128 != 0, else 128 x 128, as in the network.
 *  Size limits, r50_op_conv2d_w2: n*ho*wo <= 2^30; n*h*w*cin*2 + (pad*w+pad)*cin*2 < 2^31; n*ho*wo*cout*2 < 2^31; cout*k*k*2*cin*2 < 2^31 (the pair).
 *  Size limits, r50_op_conv2d_split: every pixel is a pair, so half the images: n*ho*wo <= 2^30; n*h*w*2*cin*2 + (pad*w+pad)*2*cin*2 < 2^31;
 *    n*ho*wo*2*cout*2 < 2^31; cout*k*k*3*cin*2 < 2^31. */
int r50_op_conv2d_w2(const void* R50_ALIGNED(16) x_nhwc_bf16, int n, int h, int w, int cin, const void* R50_ALIGNED(16) w_pair_bf16, const float* R50_ALIGNED(16) bias_f32,
                     const void* R50_ALIGNED(16) residual_nhwc_bf16, void* R50_ALIGNED(16) y_nhwc_bf16, int cout, int ksize, int stride, int pad, int relu, int tile,
                     void* stream);
int r50_op_conv2d_split(const void* R50_ALIGNED(16) x_pair_bf16, int n, int h, int w, int cin, const void* R50_ALIGNED(16) w_trip_bf16, const float* R50_ALIGNED(16) bias_f32,
                        const void* R50_ALIGNED(16) residual_pair_bf16, void* R50_ALIGNED(16) y_pair_bf16, int cout, int ksize, int stride, int pad, int relu,
                        void* stream);

/* fp8 convolution (BASELINE configs[4]: CDNA4 fp8 MFMA), kernel level. OCP e4m3 activations, weights and output, fp32 accumulation on
 * v_mfma_scale_f32_16x16x128_f8f6f4 (unit block scales).  x (n,h,w,cin) fp8, w (cout,k,k,cin) fp8, residual / y (n,ho,wo,cout) fp8;
 * with per-tensor scales sx, sw, sr, sy (real value = stored value x scale):
 *   y = fp8( act( acc * oscale + residual * rscale ) ),  acc = bias_scaled + sum x*w,
 *   bias_scaled = bias / (sx*sw) (device fp32), oscale = sx*sw/sy, rscale = sr/sy; conversion saturates at +-448.
 * cin % 128 == 0, cout % 64 == 0 (128 / 256 for the wider tiles), k in {1,3}.  tile: 0 = auto or a role-specialised tile id (64|...).
 * Size limits (one byte per element; the launcher describes the tensors as 16-bit pairs and keeps the 16-bit rule for y, which is therefore
 * held to half of what its bytes would allow): n*ho*wo <= 2^30; n*h*w*cin + (pad*w+pad)*cin < 2^31; n*ho*wo*cout*2 < 2^31; cout*k*k*cin < 2^31. */
int r50_op_conv2d_fp8(const void* R50_ALIGNED(16) x_nhwc_fp8, int n, int h, int w, int cin, const void* R50_ALIGNED(16) w_ohwi_fp8, const float* R50_ALIGNED(16) bias_scaled_f32,
                      const void* R50_ALIGNED(16) residual_nhwc_fp8, void* R50_ALIGNED(16) y_nhwc_fp8, int cout, int ksize, int stride, int pad, int relu,
                      float oscale, float rscale, int tile, void* stream);

/* 1x1 conv over TWO K sources, the form the library runs conv3 + downsample + add + ReLU of a stage's first bottleneck in
 * (torchvision Bottleneck.forward: `out = conv3(out); identity = downsample(x); out += identity; relu`): y = act([W1 | W2] .
 * [x1 ; x2 sampled at stride2] + bias).  x1 (n,h,w,c1) at the output resolution, x2 (n,h2,w2,c2) with (h2-1)/stride2+1 == h;
 * wcat (cout, c1+c2) K-major; c1, c2, cout multiples of 64.  tile: 0 = auto or a role-specialised tile id (64|...). et: 0 bf16, 1 fp16.
 * Size limits: n*h*w <= 2^30; n*h*w*c1*2 < 2^31 (x1); n*h2*w2*c2*2 < 2^31 (x2, usually the largest); n*h*w*cout*2 < 2^31 (y);
 * cout*(c1+c2)*2 < 2^31 (wcat). */
int r50_op_conv1x1_cat(const void* R50_ALIGNED(16) x1, int n, int h, int w, int c1, const void* R50_ALIGNED(16) x2, int h2, int w2, int c2, int stride2,
                       const void* R50_ALIGNED(16) wcat, const float* R50_ALIGNED(16) bias_f32, void* R50_ALIGNED(16) y, int cout, int relu, int tile, int et, void* stream);

/* Stem: fp32 NCHW frames -> conv 7x7 s2 p3 (+folded bn1 bias) + ReLU -> (n,112,112,64) bf16 NHWC.
 * w_oihw_f32: (64,3,7,7) fp32 *already folded*, host pointer; bias_f32: device pointer (64).
 * scratch_dev: at least r50_stem_scratch_bytes(n) bytes of device memory.
 * Holds the host: the weights are packed into a host temporary, uploaded on `stream`, and the call synchronises `stream` once before
 * it launches (r50_forward does not: a handle keeps its packed stem weights on the device).
 * Size limits: n*28 < 2^31 -- one workgroup per image and four output rows, counted in an int; every offset inside the two kernels is 64-bit,
 * so no tensor's bytes bound n (run with y across 2^31 elements and 2^32 bytes: DESIGN.md section 4, "Size limits"). */
int64_t r50_stem_scratch_bytes(int n);
/* Element type of the hooks that have no argument for it -- r50_op_stem, r50_op_maxpool, r50_op_avgpool, r50_op_bneck_tail,
 * r50_op_bneck_block1, r50_op_bneck_block1_ds, r50_op_bneck_block2, r50_op_bneck_cat_chain: bf16, as their parameter names say.  With
 * R50_OP_ET=1 in the environment (a test knob, read per call) they run the IEEE-half instantiations that a handle in R50_PREC_FP16
 * launches: every 16-bit tensor and weight matrix is then fp16 (the stem packs its fp32 weights to fp16), same layouts. */
int r50_op_stem(const float* x_nchw_f32_dev, int n, const float* w_oihw_f32_host,
                const float* R50_ALIGNED(16) bias_f32_dev, void* R50_ALIGNED(16) scratch_dev, void* R50_ALIGNED(16) y_nhwc_bf16, void* stream);

/* MaxPool2d(3, stride 2, pad 1) on bf16 NHWC; c % 8 == 0.
 * Size limits: n*h*w*c*2 < 2^63 -- the kernel counts and addresses in 64 bits (a grid-stride loop), so only the byte offset itself bounds it;
 * run across 2^31 input elements and 2^32 input bytes ("Size limits"). */
int r50_op_maxpool(const void* R50_ALIGNED(16) x_nhwc_bf16, int n, int h, int w, int c, void* R50_ALIGNED(16) y_nhwc_bf16, void* stream);

/* Bottleneck tail in one launch: conv3 1x1 (cmid -> 4*cmid) + bn3 + identity + ReLU -> out (m,4*cmid), and the
 * next block's conv1 1x1 (4*cmid -> c1) + bn1 + ReLU -> y1n (m,c1).  Replaces, for two consecutive torchvision
 * Bottleneck blocks, `out = relu(bn3(conv3(out)) + identity)` of the first and `out = relu(bn1(conv1(x)))` of
 * the second (upstream torchvision models/resnet.py Bottleneck.forward; the reference builds them at
 * src/preprocess_resnet_features.py:207).  Shapes: cmid = 64 (layer1; c1 in {64,128}) or cmid = 128 (layer2;
 * c1 = 128, no wd/bd).
 * wd/bd NULL: `identity` is the (m,4*cmid) identity tensor.  wd/bd given (cmid = 64, the stage's first block):
 * `identity` is the block INPUT (m,64) and the identity is `downsample(x)` = bf16(wd . x + bd), computed in
 * the kernel with the same rounding as a separate launch.  All tensors bf16 NHWC with m = n*h*w pixels,
 * weights folded (cout, cin) K-contiguous, biases fp32.  cmid = 64 reproduces the two separate launches bit
 * for bit; cmid = 128 sums the second conv's K in eight slices (fp32), i.e. within rounding of them; cmid = 256
 * (c1 = 256, layer3: the chained kernel, weights packed into fragment order per call by this hook) is bit for
 * bit again.  cmid = 256 with c1 = 0 and w1 = b1 = y1n = NULL: conv3 + identity + ReLU ALONE through the same pipelined kernel (the form the
 * stage's last block, layer3.5, runs in; bit for bit a 1x1 r50_op_conv2d with a residual).  (Environment R50_TAIL3_BP = 1..112: pixels per tile
 * of the cmid = 256 kernel; a test knob.)
 * Size limits: m*4*cmid*2 < 2^31 -- the bytes of `out`, the largest tensor of every form (with the downsample, and with c1 = 0, too): m*512 < 2^31
 * for cmid 64, m*1024 for cmid 128, m*2048 for cmid 256.  Any m up to that, a multiple of the pixel tile or not. */
int r50_op_bneck_tail(const void* R50_ALIGNED(16) y2_bf16, int64_t m, int cmid, const void* R50_ALIGNED(16) w3_bf16, const float* R50_ALIGNED(16) b3,
                      const void* R50_ALIGNED(16) identity_bf16, const void* R50_ALIGNED(16) wd_bf16, const float* R50_ALIGNED(16) bd, void* R50_ALIGNED(16) out_bf16, const void* R50_ALIGNED(16) w1_bf16,
                      int c1, const float* R50_ALIGNED(16) b1, void* R50_ALIGNED(16) y1n_bf16, void* stream);

/* A whole bottleneck BODY of layer2 (blocks .1-.3, 28x28, 128 mid channels) in one launch: t2 = relu(conv2_3x3(t1) + b2) stays in LDS,
 * out = relu(w3 . t2 + b3 + identity) and, when w1 / b1 / y1n are given, y1n = relu(w1 . out + b1) (the next block's conv1) --
 * `Bottleneck.forward` of torchvision's ResNet-50 from its second conv on (src/preprocess_resnet_features.py:296 calls it through
 * nn.Sequential).  t1 (n,28,28,128), identity / out (n,28,28,512), y1n (n,28,28,128) bf16 NHWC; w2 (128,3,3,128), w3 (512,128),
 * w1 (128,512) folded bf16, K contiguous; biases fp32.  Bit for bit what r50_op_conv2d (3x3, input-resident tile) followed by two
 * r50_op_conv2d 1x1 launches give.  w1 = b1 = y1n = NULL: no next conv1 (the stage's last block).
 * Size limits: n*28*28*512*2 < 2^31 (identity / out, the largest tensors), with or without w1. */
int r50_op_bneck_block2(const void* R50_ALIGNED(16) t1_bf16, int n, const void* R50_ALIGNED(16) w2_bf16, const float* R50_ALIGNED(16) b2, const void* R50_ALIGNED(16) w3_bf16, const float* R50_ALIGNED(16) b3,
                        const void* R50_ALIGNED(16) identity_bf16, void* R50_ALIGNED(16) out_bf16, const void* R50_ALIGNED(16) w1_bf16, const float* R50_ALIGNED(16) b1, void* R50_ALIGNED(16) y1n_bf16, void* stream);

/* layer1.0, the stage's first bottleneck, from its second conv on in one launch: as r50_op_bneck_block1 with c1 = 64, but the identity is the
 * DOWNSAMPLE conv of the block input computed in the kernel -- identity = bf16(wd . x + bd), rounded exactly as a separate 1x1 launch stores
 * it (torchvision `Bottleneck.forward`: `identity = self.downsample(x)`).  x (n,56,56,64) the block input, wd (256,64), bd (256).  Bit for bit
 * what the resident-weights 3x3 launch followed by r50_op_bneck_tail (cmid 64, wd / bd given) give.
 * Size limits: n*56*56*256*2 < 2^31 (out, the largest tensor), as r50_op_bneck_block1. */
int r50_op_bneck_block1_ds(const void* R50_ALIGNED(16) t1_bf16, int n, const void* R50_ALIGNED(16) w2_bf16, const float* R50_ALIGNED(16) b2, const void* R50_ALIGNED(16) w3_bf16, const float* R50_ALIGNED(16) b3,
                           const void* R50_ALIGNED(16) x_bf16, const void* R50_ALIGNED(16) wd_bf16, const float* R50_ALIGNED(16) bd, void* R50_ALIGNED(16) out_bf16, const void* R50_ALIGNED(16) w1_bf16, const float* R50_ALIGNED(16) b1,
                           void* R50_ALIGNED(16) y1n_bf16, void* stream);

/* The TRANSITION tail of layer2.0 chained with layer2.1.conv1 in one launch: out = relu([W3 | Wd] . [t2 ; x at stride 2] + (b3 + bd)) -- conv3,
 * the downsample conv, the add and the ReLU of torchvision's first Bottleneck of a stage (`out = relu(bn3(conv3(out)) + downsample(x))`,
 * src/preprocess_resnet_features.py:296 through nn.Sequential) as one 1x1 conv over two K sources, as r50_op_conv1x1_cat computes it -- and
 * y1n = relu(w1 . out + b1), the next block's conv1.  t2 (n,ow,ow,128), x (n,2ow,2ow,256), out (n,ow,ow,512), y1n (n,ow,ow,128) bf16 NHWC;
 * wcat (512, 128 + 256) = [W3 | Wd], w1 (128,512) folded bf16, K contiguous; bcat = b3 + bd, b1 fp32.  ow = 28.  Bit for bit what
 * r50_op_conv1x1_cat followed by a 1x1 r50_op_conv2d give.
 * Size limits: n*(2*ow)*(2*ow)*256*2 < 2^31 (x, the decisive one) and n*ow*ow*512*2 < 2^31 (out). */
int r50_op_bneck_cat_chain(const void* R50_ALIGNED(16) t2_bf16, const void* R50_ALIGNED(16) x_bf16, int n, int ow, const void* R50_ALIGNED(16) wcat_bf16, const float* R50_ALIGNED(16) bcat, void* R50_ALIGNED(16) out_bf16,
                           const void* R50_ALIGNED(16) w1_bf16, const float* R50_ALIGNED(16) b1, void* R50_ALIGNED(16) y1n_bf16, void* stream);

/* The same for layer1 (blocks .1 / .2, 56x56, 64 mid channels): t1 (n,56,56,64), identity / out (n,56,56,256), w2 (64,3,3,64), w3 (256,64),
 * w1 (c1,256) with c1 = 64 (the next layer1 block's conv1) or 128 (layer2.0.conv1), y1n (n,56,56,c1).  Bit for bit what the
 * resident-weights 3x3 launch followed by two r50_op_conv2d 1x1 launches give.
 * Size limits: n*56*56*256*2 < 2^31 (identity / out, the largest tensors), for either c1. */
int r50_op_bneck_block1(const void* R50_ALIGNED(16) t1_bf16, int n, const void* R50_ALIGNED(16) w2_bf16, const float* R50_ALIGNED(16) b2, const void* R50_ALIGNED(16) w3_bf16, const float* R50_ALIGNED(16) b3,
                        const void* R50_ALIGNED(16) identity_bf16, void* R50_ALIGNED(16) out_bf16, const void* R50_ALIGNED(16) w1_bf16, int c1, const float* R50_ALIGNED(16) b1, void* R50_ALIGNED(16) y1n_bf16, void* stream);

/* Frame producer, the step before the path: crop box + bilinear resize of a decoded clip on the
 * device.  Replaces `_crop_and_resize_video_uint8` (src/dataset.py:141-149) up to, not including, the `/255`:
 * frames (t,h,w,3) uint8 HWC as the video decoder returns them -> `frames[:, top:top+hh, left:left+ww]` ->
 * resize to (out_size,out_size), bilinear, no antialias -> out (t,3,out_size,out_size) uint8 NCHW, the input of
 * r50_forward_u8.  mode R50_RESIZE_FLOAT: the arithmetic of `torchvision.transforms.functional.resize` (the v1 API
 * the reference imports, :13): uint8 -> fp32, ATen bilinear (align_corners=False), round half to even, uint8.
 * mode R50_RESIZE_FIXED: ATen's native uint8 kernel (what the v2 API runs on an AVX2 CPU): two-pass int16 fixed
 * point with a uint8 intermediate, bit-exact.  The box comes from `_compute_square_crop_from_2d` (:75-104; host
 * code, mirrored in frames.py) and must lie inside the frame; out_size % 4 == 0.  Device pointers; asynchronous on
 * `stream` (indices and weights are computed in the kernel).  frames may sit at any byte address (each source row is staged as dwords
 * from the 4-byte boundary at or below the ADDRESS of its first byte); out is stored one dword per 4 pixels: R50_ALIGNED(4).
 * flags: the two augmentation variants that are index permutations, applied to the output exactly as
 * the reference applies them to the resized clip: R50_AUG_HFLIP = `torch.flip(video, dims=[-1])` (`_aug_hflip`, :158-166),
 * R50_AUG_TREV = `torch.flip(video, dims=[0])` (`_aug_temporal_reverse`, :199-207); joints / intrinsics are host code. */
#define R50_RESIZE_FLOAT 0
#define R50_RESIZE_FIXED 1
#define R50_AUG_HFLIP 1
#define R50_AUG_TREV 2
int r50_op_crop_resize_u8(const void* R50_ALIGNED(1) frames_thwc_u8, int t, int h, int w, int top, int left, int hh, int ww,
                          void* R50_ALIGNED(4) out_tchw_u8, int out_size, int mode, int flags, void* stream);

/* Results dump (`src/results.py`): whole-frame resize of one clip's video.  frames (n,h,w,3) uint8 HWC on the device, the decoded
 * frames the clip names; src_idx (t) int32 on the device, output frame i = frames[src_idx[i]] (the host folds `[::skip][start:end]`
 * and `_pad_or_trim_video`'s repeat-the-last-frame padding into the map, :65-79,96-116) -> out (t,out_size,out_size,3) uint8 HWC,
 * contiguous (may be one clip's slice of a (B,t,out_size,out_size,3) buffer).  Arithmetic of `_resize_video_hw` (:81-93): fp32
 * u8 / 255 (IEEE division), bilinear with align_corners=False and no antialias as F.interpolate's CPU path evaluates it for 3
 * channels, clamp(0,1) * 255, truncated to uint8 (not rounded: unlike both R50_RESIZE_* modes).  Any out_size >= 1.  src_idx is
 * read back once to check every index lies in [0,n) (R50_ERR_INVALID otherwise): the call synchronises `stream` once, so it
 * holds the host until everything queued on `stream` before it has run.  Of the r50_op_* entry points only this one and r50_op_stem
 * do (tests/test_stream_order_gpu.py, BLOCKS_HOST). */
int r50_op_resize_frames_u8(const void* R50_ALIGNED(1) frames_nhwc_u8, int n, int h, int w, const int* src_idx, int t, void* R50_ALIGNED(1) out_tssc_u8,
                            int out_size, void* stream);

/* Results rendering (no counterpart in the reference, whose src/visualize_2d.py draws with matplotlib on the
 * host): anti-aliased skeleton layers blended over uint8 frames.  bg (f,h,w,3) uint8 HWC on the device, or NULL for the uniform colour
 * bg_rgb = 0xRRGGBB; pts (f,layers,joints,2) fp32 on the device, pixel coordinates, x first: pixel (row i, col j) has its centre at
 * (x = j, y = i), the convention under which matplotlib overlays `scatter` on `imshow`; style (f,layers,4) uint8 on the device = R, G,
 * B, A per frame and layer, A = 0 switches the layer off for that frame; edges_host: 2*n_edges ints ON THE HOST, pairs of joint indices
 * (they travel as kernel arguments: no allocation, no synchronisation); out (f,h,w,3) uint8, which may not overlap bg.
 * Per pixel p, the layers l = 0 .. layers-1 in order (later layers on top):
 *   d_e = the smallest distance from p to a segment whose two end points are finite (a segment of zero length is a point),
 *   d_j = the smallest distance from p to a finite joint; a joint with a NaN or inf coordinate is skipped, and so is every edge at it;
 *   a   = max(clamp(half_width + 0.5 - d_e, 0, 1), clamp(joint_radius + 0.5 - d_j, 0, 1)) * A / 255,
 *   c   = c * (1 - a) + rgb * a per channel in fp32, starting from the background byte; out = floor(c + 0.5) clamped to 0..255.
 * A pixel with a == 0 in every layer leaves as its background byte.  Distances are formed in fp64 from the differences (p - a); the
 * coverage, alpha and blend are fp32.  Coordinates of magnitude up to 2^20 keep that accuracy; larger finite ones are legal (nothing
 * is indexed by a coordinate) but unspecified in value.  Gather form, one thread per 4 pixels, no atomics: the same bits on every run.
 * w % 4 == 0 with bg and out 4-byte aligned takes a 12-byte vector path, anything else a per-byte path; same values.
 * bg, style and out may sit at any byte address (R50_ALIGNED(1)): style is read byte by byte.
 * Refused with a message before any launch unless pts, style and out are non-NULL, f, h, w >= 1, 1 <= joints <= 64,
 * 1 <= layers <= 8, 0 <= n_edges <= 128 (edges_host non-NULL when n_edges > 0), every edge index in [0, joints), half_width and
 * joint_radius finite and >= 0, 0 <= bg_rgb <= 0xFFFFFF and out does not overlap bg.  Asynchronous on `stream`. */
int r50_op_draw_skeletons_u8(const void* R50_ALIGNED(1) bg_fhwc_u8, int bg_rgb, const float* pts_flj2_f32, const void* R50_ALIGNED(1) style_fl4_u8,
                             const int* edges_host, int n_edges, int f, int h, int w, int layers, int joints, float half_width,
                             float joint_radius, void* R50_ALIGNED(1) out_fhwc_u8, void* stream);

/* ColorJitter augmentation variant: `_aug_color_jitter` (src/dataset.py:188-197) = torchvision.transforms.v2
 * ColorJitter(brightness=0.3, contrast=0.3, saturation=0.2, hue=0.05) on the float clip in [0,1], followed (normalize != 0) by
 * `frame_tf` = Normalize(ImageNet mean, std) (:242-245).  frames_u8: (t,3,hw) uint8 resized crops on the device (the output of
 * r50_op_crop_resize_u8); order4: the sampled permutation of {0 brightness, 1 contrast, 2 saturation, 3 hue} (HOST pointer); the
 * four factors as sampled (host code: frames.sample_color_jitter_params); out_f32: (t,3,hw) fp32, what r50_forward takes;
 * scratch_means: t floats of device memory (per-frame grayscale mean of adjust_contrast).  Asynchronous on `stream`. */
int r50_op_color_jitter_u8(const void* R50_ALIGNED(1) frames_u8, int t, int hw, const int* order4_host, float brightness, float contrast,
                           float saturation, float hue, int normalize, float* out_f32, float* scratch_means, void* stream);

/* Lifting head, forward (first step): the non-GEMM pieces of `PHDFor3DJoints.forward` (src/model.py:146-178);
 * its Linear layers and causal conv1d's run on r50_op_conv2d / r50_op_conv2d_f16 as 1x1 convolutions over the b*t rows.
 * et: 0 = bf16, 1 = fp16.  All device pointers.
 *  r50_op_cast_rows: fp32 (rows,c) -> element (rows,cpad), zero columns beyond c (`feats` before `input_proj`, :155).
 *  r50_op_concat_pad: [phi (rows,d) element | y (rows,ny) fp32 | zeros] -> (rows,dp) element = `torch.cat([phi, y], -1)` of the
 *    iterative regressor (:113) padded to the GEMM's K granularity.
 *  r50_op_gn_relu_causal3: x (b,t,c) element -> GroupNorm(groups, eps) + ReLU (`ResidualBlock`, :47-55) -> the input rows of
 *    the following `CausalConv1d` (kernel 3, replicate left padding, :20-35): out (b*t, 3c), row (b,t) =
 *    [y(t-2) | y(t-1) | y(t)] with indices clamped at 0.
 *  r50_op_add_rows: y (rows,ny) fp32 += dy (rows,dp) element, first ny columns (`y = y + dy`, :114-115).
 * Alignment: these kernels, and the element-wise, GroupNorm and reduction ops of the training step below, read and write 16-bit tensors
 * one element at a time (R50_ALIGNED(2)) -- except r50_op_cast_rows, which stores one 4-byte pair per two columns: dst is
 * R50_ALIGNED(4), and cpad is even so that every row of dst starts on a 4-byte boundary too. */
int r50_op_cast_rows(const float* src_f32, int64_t rows, int c, void* R50_ALIGNED(4) dst, int cpad, int et, void* stream);
int r50_op_concat_pad(const void* R50_ALIGNED(2) phi, int d, const float* y_f32, int ny, int64_t rows, void* R50_ALIGNED(2) dst, int dp, int et, void* stream);
int r50_op_add_rows(float* y_f32, int ny, const void* R50_ALIGNED(2) dy, int dp, int64_t rows, int et, void* stream);
int r50_op_gn_relu_causal3(const void* R50_ALIGNED(2) x, int b, int t, int c, int groups, const float* gamma, const float* beta, float eps,
                           void* R50_ALIGNED(2) out, int et, void* stream);

/* Lifting head, autoregressive rollout: f_AR over a TIME-MAJOR sequence that grows by one frame per step.
 *  r50_op_gn_relu_causal3_tm: r50_op_gn_relu_causal3 on x (t,b,c) time-major, statistics over all t rows of each sample and
 *    group, emitting only the rows t' in [t0, t): out ((t-t0)*b, 3c), row (t'-t0)*b + b' = [y(t'-2) | y(t'-1) | y(t')] of sample b',
 *    indices clamped at 0.  0 <= t0 < t.  With t0 = 0 the values are bit-equal to r50_op_gn_relu_causal3 on the batch-major
 *    transpose (same grid, summation order and tree); t0 = t-1 emits the last row of each sample only. */
int r50_op_gn_relu_causal3_tm(const void* R50_ALIGNED(2) x, int b, int t, int t0, int c, int groups, const float* gamma, const float* beta, float eps,
                              void* R50_ALIGNED(2) out, int et, void* stream);

/* Lifting head, backward + optimizer: the training step of `train()` (src/train.py:137-176: fp16 autocast forward, `l3d` MSE
 * loss, GradScaler, AdamW).  Every matrix product of the backward pass (dX = dY W, dW = dY^T X) is an r50_op_conv2d(_f16) launch
 * on operands transposed by r50_op_transpose16; these are the pieces around them.  16-bit tensors are `et` elements (0 bf16, 1 fp16).
 *  r50_op_transpose16: src (rows,cols) -> dst (cols,ld), dst[c][r] = src[r][c]; ld >= rows, the padding columns are left alone.
 *  r50_op_mask_scale: x *= mask * scale in place (`nn.Dropout`, src/model.py:44,98); mask one byte per element.
 *  r50_op_relu_bwd: dy = dy * scale * (act > 0) in place (backward of ReLU, or of ReLU + dropout with act = the dropped-out tensor).
 *  r50_op_colsum / _f32: out (cols) fp32 [+]= scale * column sums of x (rows,ld)[:, :cols] (bias gradients; rows summed in order).
 *  r50_op_grad_accum: dst (n) fp32 [+]= scale * src (n) 16-bit (a weight gradient into the flat fp32 gradient buffer, unscaled).
 *  r50_op_mse_loss_grad: loss2[0] = mean((y-gt)^2) (:161), loss2[1] = MPJPE (:42-45); dy = 2 (y-gt) / n * loss_scale; n = B*T*J*3.
 *  r50_op_gn_relu_causal3_bwd: backward of r50_op_gn_relu_causal3: dr (b*t,3c) -> dx (b,t,c) [+ add], per-sample parameter
 *    gradient parts dgamma_part / dbeta_part (b,c) fp32 (sum over b with r50_op_colsum_f32).
 *  r50_op_check_finite: found[0] |= any non-finite in g (GradScaler's inf check, :172-174).
 *  r50_op_check_overflow16: found[0] |= any inf / nan in 16-bit x -- or, for fp16, any element at +-65504: the fp32 -> fp16 conversion
 *    of this library saturates instead of producing inf, so that is what an overflowed gradient looks like.
 *  r50_op_adamw: `torch.optim.AdamW` (:389) over flat fp32 p / m / v / g, step >= 1; skipped when found_inf[0] != 0; p16 = the
 *    refreshed 16-bit copy of p the GEMMs read. */
int r50_op_transpose16(const void* R50_ALIGNED(2) src, int rows, int cols, void* R50_ALIGNED(2) dst, int ld, void* stream);
int r50_op_mask_scale(void* R50_ALIGNED(2) x, const void* R50_ALIGNED(1) mask_u8, float scale, int64_t n, int et, void* stream);
int r50_op_relu_bwd(void* R50_ALIGNED(2) dy, const void* R50_ALIGNED(2) act, float scale, int64_t n, int et, void* stream);
int r50_op_colsum(const void* R50_ALIGNED(2) x, int64_t rows, int cols, int ld, float scale, float* out_f32, int accumulate, int et, void* stream);
int r50_op_colsum_f32(const float* x, int64_t rows, int cols, float scale, float* out_f32, int accumulate, void* stream);
int r50_op_grad_accum(const void* R50_ALIGNED(2) src, float scale, float* dst_f32, int64_t n, int accumulate, int et, void* stream);
int r50_op_mse_loss_grad(const float* y, const float* gt, int64_t n, float loss_scale, float* dy, float* loss2, void* stream);
int r50_op_gn_relu_causal3_bwd(const void* R50_ALIGNED(2) dr, const void* R50_ALIGNED(2) x, int b, int t, int c, int groups, const float* gamma, const float* beta,
                               float eps, const void* R50_ALIGNED(2) add, void* R50_ALIGNED(2) dx, float* dgamma_part, float* dbeta_part, int et, void* stream);
int r50_op_check_finite(const float* g, int64_t n, int* found, void* stream);
int r50_op_check_overflow16(const void* R50_ALIGNED(2) x, int64_t n, int* found, int et, void* stream);
int r50_op_adamw(float* p, float* m, float* v, const float* g, void* R50_ALIGNED(2) p16, int64_t n, float lr, float beta1, float beta2, float eps,
                 float weight_decay, int step, const int* found_inf, int et, void* stream);

/* Global-norm gradient clipping and EMA weights: the tail of a step when either is switched on.
 *  r50_op_grad_norm: the L2 norm of g (n fp32), GradScaler's finite check and `torch.nn.utils.clip_grad_norm_`'s coefficient in ONE
 *    read of g; it takes the place of r50_op_check_finite.  Two launches.  The first forms part[w], the fp64 sum of squares of
 *    workgroup w's contiguous slice: W = min(ceil(n / 4096), 2048) workgroups, slices of ceil(n / W) rounded up to a multiple of 4
 *    -- a function of n alone, never of the device -- per-thread fp64 partials over a fixed stride (the product of two fp32 values is
 *    exact in fp64), a fixed shuffle / LDS tree, no atomics.  The second (one workgroup) adds part[0..W) in a fixed order.  A sum that
 *    is not finite sets found[0] = 1 (exactly when r50_op_check_finite would: an fp64 sum of at most 2^40 fp32 squares cannot
 *    overflow) and writes clip2 = {1, float(sqrt(sum))}; found is never cleared.  Otherwise norm = sqrt(sum),
 *    coef = min(1, max_norm / (norm + 1e-6)) in fp64 (max_norm <= 0: coef = 1, norm and flag only), clip2 = {float(coef),
 *    float(norm)}, and, when found[0] is still 0, stats4 = {steps, steps with coef < 1, sum of norms, largest norm} (device doubles,
 *    zeroed by the caller) moves.  part: n_part >= W doubles of scratch; g 16-byte aligned.  The same bits on every run.
 *  r50_op_adamw_clip_ema: r50_op_adamw with g[i] * clip[0] (one fp32 product) in the place of g[i] when clip is not NULL, and, when
 *    ema is not NULL, ema[i] += ema_weight * (p_new[i] - ema[i]) (each operation rounded once: the lerp form of
 *    `torch.optim.swa_utils.get_ema_multi_avg_fn`).  With both NULL the bits are r50_op_adamw's.  Skipped as a whole when
 *    found_inf[0] != 0.  g is NOT written: it keeps the unclipped gradient. */
int r50_op_grad_norm(const float* R50_ALIGNED(16) g, int64_t n, float max_norm, double* part, int n_part, int* found, float* clip2, double* stats4,
                     void* stream);
int r50_op_adamw_clip_ema(float* p, float* m, float* v, const float* g, void* R50_ALIGNED(2) p16, int64_t n, float lr, float beta1, float beta2, float eps,
                          float weight_decay, int step, const int* found_inf, const float* clip, float* ema, float ema_weight, int et,
                          void* stream);

/* Lifting head, evaluation (`evaluate()`, src/train.py:219-280): pred, gt (rows, joints, 3) fp32 -> acc[0] += mean((pred-gt)^2)
 * (l3d, :259), acc[1] += mean over the rows*joints joints of |pred-gt|_2 (MPJPE, :42-45), acc[2] += 1; acc: 3 doubles of device
 * memory, so the mean over per-batch means is acc[0..1] / acc[2].  fp32 per joint, fp64 sums in a fixed order (no atomics: the
 * same bits on every run).  One launch of one workgroup, sized for up to ~1e5 joints per batch. */
int r50_op_pose_metrics(const float* pred, const float* gt, int64_t rows, int joints, double* acc, void* stream);

/* Lifting head, forecasting metrics of a rollout: pred (b,p,joints,3) fp32 predicts frames i0 .. i0+p-1
 * of gt (b,t_gt,joints,3) fp32; i0 + p <= t_gt.  ADDS acc[k] += sum over clips and joints of |pred[:,k]-gt[:,i0+k]|_2 (MPJPE sum),
 * acc[p+k] += the sum of squared errors, acc[2p] += b; acc: 2p+1 doubles of device memory.  One workgroup per horizon, fp32 per
 * joint, fp64 sums in a fixed order (no atomics: the same bits on every run). */
int r50_op_horizon_metrics(const float* pred, const float* gt, int b, int p, int t_gt, int i0, int joints, double* acc, void* stream);

/* Lifting head, the H3.6M evaluation protocols per group: pred (b,p,joints,3) fp32 scores frames
 * i0 .. i0+p-1 of gt (b,t_gt,joints,3) fp32 (r50_op_horizon_metrics' indexing); group (b) int32 device values in [0,n_groups).  Per
 * pose, in fp64: P1 = mean over joints of |(pred_j - pred_root) - (gt_j - gt_root)|, P2 = the same distance after the least-squares
 * proper similarity fit of pred onto gt (Umeyama 1991; scale 0 when either pose has no spread).  ADDS acc[(g*p + k)*2 + 0] += the P1
 * sum and acc[(g*p + k)*2 + 1] += the P2 sum over the clips of group g at frame k, acc[2*n_groups*p + g] += the clips of group g;
 * acc: 2*n_groups*p + n_groups doubles of device memory.  Needs b, p, n_groups >= 1, 1 <= joints <= 64, 0 <= root < joints,
 * 0 <= i0, i0 + p <= t_gt; checked before any launch.  One workgroup per (frame, group), one whole pose per thread, fp64 sums in a
 * fixed order (no atomics: the same bits on every run). */
int r50_op_pose_protocols(const float* pred, const float* gt, const int* group, int b, int p, int t_gt, int i0, int joints, int root,
                          int n_groups, double* acc, void* stream);

/* Lifting head, detail metrics per group: per-joint errors, PCK / AUC hit counts and velocity /
 * acceleration errors, with r50_op_pose_protocols' indexing (pred (b,p,joints,3) fp32 scores frames i0 .. i0+p-1 of gt
 * (b,t_gt,joints,3) fp32; group (b) int32 device values in [0,n_groups)).  Read as fp32, computed in fp64.  Per clip, scored frame k
 * and joint j, with ~ for root-relative (pred_j - pred_root): d1 = |~pred_j - ~gt_j| (P1's term); d2 = |a R (pred_j - mu_pred) +
 * mu_gt - gt_j| with (a, R) the proper similarity fit of r50_op_pose_protocols (P2's term); ev = |(~pred[k] - ~pred[k-1]) -
 * (~gt[k] - ~gt[k-1])| for k >= 1, in metres per frame; ea = |(~pred[k-1] - 2 ~pred[k] + ~pred[k+1]) - (the same of ~gt)| for
 * 1 <= k <= p-2, in metres per frame^2: differences are taken inside pred, no frame rate is assumed.  Thresholds tau_i = thr_max * i /
 * (n_thr - 1), i = 0 .. n_thr-1, in fp64 in that order; d hits tau when d < tau (strict: tau_0 = 0 is never hit, an exact 0 hits
 * every positive threshold).  With G = n_groups, P = p, J = joints and A = 2*G*P*J it ADDS
 *   acc[((g*P + k)*J + j)*2 + {0,1}]   += the sums over the clips of group g of d1, d2;
 *   acc[A + (g*P + k)*6 + {0,1,2,3}]   += over clips and joints: the hits of d1 summed over all n_thr thresholds, the hits of d1 at
 *                                         thr_max, then the same two of d2 (integer-valued);
 *   acc[A + (g*P + k)*6 + {4,5}]       += the sums over clips and joints of ev, ea; nothing where they are undefined;
 *   acc[A + 6*G*P + g]                 += the clips of group g;
 * acc: 2*G*P*J + 6*G*P + G doubles of device memory.  Needs b, p, n_groups >= 1, 1 <= joints <= 64, 0 <= root < joints, 0 <= i0,
 * i0 + p <= t_gt, 2 <= n_thr <= 1024, thr_max > 0 and finite, no null pointer; all checked before any launch (a refused call touches
 * nothing).  One workgroup per (frame, group), one fit per thread, fp64 sums in a fixed order (no atomics: the same bits on every
 * run). */
int r50_op_pose_detail_metrics(const float* pred, const float* gt, const int* group, int b, int p, int t_gt, int i0, int joints, int root,
                               int n_groups, int n_thr, double thr_max, double* acc, void* stream);

/* Lifting head, forecast error after dynamic time warping per group: pred (b,p,joints,3) fp32 holds the
 * predicted poses Y_0..Y_{p-1} of each clip, X_0..X_{q-1} are frames i0 .. i0+q-1 of gt (b,t_gt,joints,3) fp32; group (b) int32 device
 * values in [0,n_groups).  Read as fp32, computed in fp64.  Per clip two cost matrices, C1[i][j] = P1 and C2[i][j] = P2 of (Y_i, X_j)
 * as r50_op_pose_protocols defines them, one similarity fit per cell giving both.  band < 0 allows every cell, band >= 0 the cells
 * with |i - j| <= band; a band >= 0 below |p - q| is refused.  Per metric a closed-ended DP: D[0][0] = C[0][0], D[i][j] = C[i][j] +
 * the best predecessor among (i-1,j-1), (i-1,j), (i,j-1) that exist and are allowed, taken in that order, a later candidate replacing
 * the current one only if strictly smaller: ties go diagonal, then up, then left, and a NaN never replaces anything.  The path is the
 * backtrack of the stored choices from (p-1,q-1) to (0,0); its length L lies in [max(p,q), p+q-1].  Every loop is bounded by p, q,
 * p*q or p+q: non-finite input gives non-finite sums, never a hang.  Per clip and metric m (0 = P1, 1 = P2): total = D[p-1][q-1]; L;
 * cost_sum[k] = the sum of C[i][j], cells[k] = the count and lag_sum[k] = the sum of (i - j) over the path cells with i = k.  The DTW
 * error of a clip is total / L, at horizon k cost_sum[k] / cells[k]; the lag at horizon k is lag_sum[k] / cells[k] frames, positive
 * when the prediction runs behind the ground truth's clock (it is slow).
 *   clip_out (b, 2, 2 + 3p) doubles, always WRITTEN: [total, L, cost_sum[p], cells[p], lag_sum[p]] per clip and metric;
 *   path_out may be null; otherwise (b, 2, p+q-1, 2) int32, WRITTEN: the path's (i, j) pairs from (0,0) onward, -1 past L;
 *   acc: n_groups*2*(1 + 2p) + n_groups doubles; with V = 1 + 2p it ADDS over the clips of group g
 *     acc[(g*2 + m)*V + 0] += total / L,  acc[(g*2 + m)*V + 1 + k] += cost_sum[k] / cells[k],
 *     acc[(g*2 + m)*V + 1 + p + k] += lag_sum[k] / cells[k],  acc[2*n_groups*V + g] += the clips of group g.
 * Needs b, n_groups >= 1, 1 <= p, q <= 64, 1 <= joints <= 64, 0 <= root < joints, 0 <= i0, i0 + q <= t_gt, no null pointer but
 * path_out; all checked before any launch (a refused call touches nothing).  Two launches on stream: one workgroup per clip (cost
 * matrices, DP state and choices in LDS), then one workgroup per group; fixed summation order, no atomics: the same bits on every run. */
int r50_op_dtw_protocols(const float* pred, const float* gt, const int* group, int b, int p, int t_gt, int i0, int q, int joints, int root,
                         int band, int n_groups, double* clip_out, int* path_out, double* acc, void* stream);

/* Dense evaluation, the fusion of overlapping clips into one pose per video frame: pred, gt
 * (rows/t, t, joints, 3) fp32 seen as rows = N*t pose rows; output frame f has the contributors src[offsets[f] .. offsets[f+1]), each a
 * row index item*t + t_c, read in list order; offsets (frames+1) and src int32 device values.  Per frame with n contributors, in fp64
 * with one rounding to fp32 at each store:
 *   fused (frames,joints,3)  = sum_c w_c pred_c / sum_c w_c with w_c = 1 (mode 0, mean) or min(t_c + 1, ramp) (mode 1, context); mode 2
 *                              (last) copies the contributor with the greatest t_c, the first in list order on a tie, bit for bit;
 *   gt_out (frames,joints,3) = the first contributor's gt row, copied;
 *   spread (frames)          = sqrt(sum_c sum_j |pred_cj - m_j|^2 / (joints n)), m the unweighted mean: the same in every mode, 0 for n = 1;
 *   gt_gap (frames)          = the largest |gt_c - gt_first| over contributors and components (0 when the index is right).
 * An empty list writes zeros.  Needs 1 <= rows < 2^31 a multiple of t >= 1, 1 <= joints <= 64, frames >= 1, mode in {0,1,2}, ramp >= 1,
 * no null pointer; checked before any launch.  The kernel TRUSTS offsets and src: the caller checks on the host that offsets is
 * non-decreasing from 0 to the length of src and that every src lies in [0, rows).  Gather form, one wave per output frame, no atomics:
 * the same bits on every run. */
int r50_op_stitch_poses(const float* pred, const float* gt, int64_t rows, int joints, const int* offsets, const int* src, int frames, int t,
                        int mode, int ramp, float* fused, float* gt_out, float* spread, float* gt_gap, void* stream);

/* Dense evaluation, per-frame errors of stitched sequences per group: fused, gt (frames,joints,3) fp32, spread
 * (frames) fp32, offsets (frames+1), and per frame row its sequence seq, sub-frame index idx and group in [0,n_groups), all int32 device
 * values (a row with another group value is counted nowhere).  Row r has a velocity term if row r-1 has the same seq and idx[r-1] ==
 * idx[r] - 1, an acceleration term if row r+1 continues the sequence as well; P1, velocity and acceleration errors are those of
 * r50_op_pose_detail_metrics, per pose (means over joints, root-relative).  Workgroup b of n_blocks owns the rows [b*chunk, (b+1)*chunk),
 * chunk = ceil(frames / n_blocks), and WRITES (does not add)
 *   part[(b*n_groups + g)*8 + {0..7}] = [frames, sum P1, velocity terms, sum velocity error, acceleration terms, sum acceleration error,
 *                                        sum spread, frames with >= 2 contributors] of its rows of group g;
 * part: n_blocks*n_groups*8 doubles of device memory; the caller sums the blocks in block order.  Needs frames, n_groups, n_blocks >= 1,
 * 1 <= joints <= 64, 0 <= root < joints, no null pointer; checked before any launch.  fp64 sums in a fixed order (no atomics: the same
 * bits on every run). */
int r50_op_sequence_metrics(const float* fused, const float* gt, const float* spread, const int* offsets, const int* seq, const int* idx,
                            const int* group, int frames, int joints, int root, int n_groups, double* part, int n_blocks, void* stream);

/* Video in, poses out: the two device steps of the pass that nothing else provides.
 *  r50_op_gather_window_rows: the head's windows are views of one feature matrix.  src_f32 (src_rows, c) fp32, starts (b) int32
 *    device values, dst (b*t, c) elements (et 0 = bf16, 1 = fp16): dst row w*t + i = the cast of src row starts[w] + i, with
 *    r50_op_cast_rows' rounding and saturation, so the result is bit-equal to r50_op_cast_rows of the gathered fp32 rows without that
 *    (b*t, c) fp32 intermediate.  Windows may overlap and repeat.  Needs b >= 1, 1 <= t <= src_rows < 2^31, c a positive multiple of
 *    8, b * t * c / 8 < 2^31, src and dst 16-byte aligned, no null pointer; checked before any launch.  The kernel TRUSTS starts: the
 *    caller checks on the host that every start lies in [0, src_rows - t].  Each lane moves 8 columns: two 16-byte loads, one 16-byte
 *    store; grid-stride.
 *  r50_op_merge_mirrored_poses: flip test-time augmentation.  a, out (rows, joints, 3) fp32 = the poses of the frames as they are,
 *    b_mirrored the poses of the horizontally mirrored frames; perm (joints) int32 device values, the left/right joint swap.
 *    out[r,j,k] = 0.5f * (a[r,j,k] + s_k * b_mirrored[r,perm[j],k]), s = (-1, 1, 1): the add and the multiply are two fp32
 *    operations, each rounded to nearest even.  Needs rows >= 1, 1 <= joints <= 64, no null pointer, out either exactly a or
 *    overlapping neither input; checked before any launch.  The kernel TRUSTS perm: the caller checks on the host that every entry
 *    lies in [0, joints) and that perm[perm[j]] == j.  No atomics: the same bits on every run. */
int r50_op_gather_window_rows(const float* R50_ALIGNED(16) src_f32, int64_t src_rows, int c, const int* starts, int b, int t, void* R50_ALIGNED(16) dst, int et,
                              void* stream);
int r50_op_merge_mirrored_poses(const float* a, const float* b_mirrored, int64_t rows, int joints, const int* perm, float* out,
                                void* stream);

/* Lifting head, phase 2 (training f_AR; DESIGN.md "f next #2").  The reference has no phase 2; this
 * project's definition: f_movie / f_3D frozen and run as at inference, loss = l3d_hat + lambda * l_lat over frames s >= 1.
 *  r50_op_future_pose_loss_grad: y_hat, gt, dy (b*t, joints, 3) fp32: dy = 2 (y_hat-gt) / n * loss_scale with n = b*(t-1)*joints*3,
 *    dy = 0 on frame 0 of every clip; loss2[0] = l3d_hat = mean over s >= 1 of (y_hat-gt)^2, loss2[1] = MPJPE over s >= 1.
 *  r50_op_ar_latent_grad: ar (b,t,d) et = f_AR's output, phi (b,t,d) et = the teacher, dphi_hat (b,t,d) fp32 = the gradient that
 *    reached phi_hat (the regressor's dX).  dar (b,t,d) et = cast16(dphi_hat[b,s+1] + lambda * 2 (ar[b,s] - phi[b,s+1]) / n_l *
 *    loss_scale) for s <= t-2 and 0 for s = t-1, n_l = b*(t-1)*d; loss_lat[0] = mean (ar[b,s] - phi[b,s+1])^2 (fp32, one value);
 *    row_part: b*t floats of device scratch.  Needs t >= 2, d % 8 == 0, ar / phi / dphi_hat / dar 16-byte aligned.
 * Both reductions sum in a fixed order without atomics: the same bits on every run.  Arguments are checked before any launch. */
int r50_op_future_pose_loss_grad(const float* y_hat, const float* gt, int b, int t, int joints, float loss_scale, float* dy, float* loss2,
                                 void* stream);
int r50_op_ar_latent_grad(const void* R50_ALIGNED(16) ar, const void* R50_ALIGNED(16) phi, const float* R50_ALIGNED(16) dphi_hat, int b, int t, int d, float lambda, float loss_scale,
                          void* R50_ALIGNED(16) dar, float* loss_lat, float* row_part, int et, void* stream);

/* Lifting head, joint training (input_proj, f_movie, f_AR and f_3D under one loss).
 *  r50_op_joint_pose_loss_grad: y, dy (2*b*t, joints, 3) fp32, the regressor's output on [phi ; phi_hat] stacked by rows; gt
 *    (b, t, joints, 3) fp32.  First half: dy = 2 (y-gt) / n1 * loss_scale, n1 = b*t*joints*3 (r50_op_mse_loss_grad's arithmetic).
 *    Second half: dy = 2 (y-gt) / n2 * (loss_scale * lambda_future), n2 = b*(t-1)*joints*3, exact 0 on frame 0 of every clip
 *    (r50_op_future_pose_loss_grad's arithmetic).  out4 = [l3d, mpjpe over all frames, l3d_hat, mpjpe_hat over frames s >= 1].  One
 *    launch; fp64 sums in a fixed order without atomics (the same bits on every run).  Needs b >= 1, t >= 2, 1 <= joints <= 64;
 *    checked before any launch.
 *  r50_op_colsum_split: r50_op_colsum's result bit for bit (the same summation order and roundings), its 16 row chains per column
 *    spread over 16 x ceil(cols/64) workgroups with loads in flight, then summed in order by a second launch; part: 16*cols floats
 *    of device scratch.  The joint step's bias gradients, over up to 2*b*t rows. */
int r50_op_colsum_split(const void* R50_ALIGNED(2) x, int64_t rows, int cols, int ld, float scale, float* part, float* out_f32, int accumulate, int et,
                        void* stream);
int r50_op_joint_pose_loss_grad(const float* y, const float* gt, int b, int t, int joints, float lambda_future, float loss_scale, float* dy,
                                float* out4, void* stream);

/* Lifting head, rollout training (f_AR trained on its own multi-step rollouts).  Time-major buffers: row
 * h*b + b' is frame (or horizon) h of sample b'.
 *  r50_op_gn_relu_causal3_tm_bwd: backward of r50_op_gn_relu_causal3_tm.  dr ((t-t0)*b, 3c) = the gradient of exactly the rows the
 *    forward emitted; x, dx (t*b, c) time-major, dx over ALL t frames [+ add (t*b, c)]; dgamma_part / dbeta_part (b,c) fp32 as in
 *    r50_op_gn_relu_causal3_bwd.  0 <= t0 < t, c % groups == 0, c / groups <= 256.  With t0 = 0 the result is bit-equal to
 *    r50_op_gn_relu_causal3_bwd on the batch-major transpose.
 *  r50_op_rollout_pose_loss_grad: pred (k*b, joints, 3) fp32 time-major against gt (b, t_gt, joints, 3) fp32 at frames i0 .. i0+k-1:
 *    dy (k*b, joints, 3) = 2 (pred - gt) / n * loss_scale, n = k*b*joints*3; loss2 = [mean squared error, MPJPE] over the k horizons.
 *  r50_op_rollout_latent_grad: fut (k*b, d) et time-major against the teacher phi (b, t_phi, d) et batch-major at frames i0 ..:
 *    dfut (k*b, d) fp32 += lambda * 2 (fut - phi) / n_l * loss_scale, n_l = k*b*d; loss_lat[0] = mean (fut - phi)^2; row_part: k*b
 *    floats of device scratch.  d % 8 == 0; fut, phi and dfut 16-byte aligned.
 * The reductions sum in a fixed order without atomics: the same bits on every run.  Arguments are checked before any launch. */
int r50_op_gn_relu_causal3_tm_bwd(const void* R50_ALIGNED(2) dr, const void* R50_ALIGNED(2) x, int b, int t, int t0, int c, int groups, const float* gamma,
                                  const float* beta, float eps, const void* R50_ALIGNED(2) add, void* R50_ALIGNED(2) dx, float* dgamma_part, float* dbeta_part, int et,
                                  void* stream);
int r50_op_rollout_pose_loss_grad(const float* pred, const float* gt, int b, int k, int t_gt, int i0, int joints, float loss_scale,
                                  float* dy, float* loss2, void* stream);
int r50_op_rollout_latent_grad(const void* R50_ALIGNED(16) fut, const void* R50_ALIGNED(16) phi, int b, int k, int t_phi, int i0, int d, float lambda, float loss_scale,
                               float* R50_ALIGNED(16) dfut, float* loss_lat, float* row_part, int et, void* stream);

/* Lifting head, geometric losses (3D + 2D reprojection + velocity + bone length).
 *  r50_op_geo_pose_loss_grad: y, dy (b*t, joints, 3) fp32 batch-major, gt3d (b,t,joints,3), gt2d (b,t,joints,2), K (b,3,3), all fp32 on
 *    the device; edges_host: 2*n_edges ints ON THE HOST (they travel as kernel arguments: no allocation, no host read of device
 *    memory, no synchronisation inside, so the op can be captured in a HIP graph).
 *      uv     = (K p)[:2] / clamp((K p)[2], min = eps)     (src/train.py:84-110; the numerator is not clamped; below the clamp the
 *                                                            denominator carries no gradient, at equality it does)
 *      l3d    = mean (p - g3d)^2                            over b*(t-s0)*joints*3
 *      l2d    = mean (uv - g2d)^2                           over b*(t-s0)*joints*2, pixels^2
 *      l_vel  = mean ((p[s+1]-p[s]) - (g[s+1]-g[s]))^2      over the pairs (s, s+1), s >= s0: b*(t-s0-1)*joints*3
 *      l_bone = mean (|p[e1]-p[e0]| - |g[e1]-g[e0]|)^2      over b*(t-s0)*n_edges (src/train.py:50-57; a predicted bone of length
 *                                                            exactly 0 gets gradient 0 from that bone)
 *      loss   = l3d + lambda_2d l2d + lambda_vel l_vel + lambda_bone l_bone
 *    Frames s < s0 (s0 = 0 or 1) of every clip are left out of every term and every mean; their dy rows are exact +0.
 *    dy = (loss_scale * term_scale) * d loss / d y, all four terms in one pass.  dy == NULL: losses only (the evaluation form; the same
 *    out8).  A term whose lambda is exactly 0 adds nothing to dy and is still reported.  With all three lambdas 0 dy is bit-equal to
 *    r50_op_mse_loss_grad's (s0 = 0) and r50_op_future_pose_loss_grad's (s0 = 1) at term_scale = 1.
 *    out8 = [loss, l3d, mpjpe, l2d, reproj_px, l_vel, l_bone, n_clamped]: reproj_px = mean |uv - g2d|_2 over the included joints,
 *    n_clamped = how many of them have (K p)[2] < eps; loss is the sum above without term_scale.  An empty mean (t - s0 == 1 for
 *    l_vel, n_edges == 0 for l_bone) is reported as 0.  part: 8*b doubles of device scratch.
 *    One workgroup per clip, gather form, no atomics; per-joint arithmetic fp32, fp64 sums in a fixed order: the same bits on every run.  Refused with a message
 *    before any launch unless b >= 1, 0 <= s0 <= 1, t - s0 >= 1 (>= 2 when lambda_vel != 0), 1 <= joints <= 64, 0 <= n_edges <= 64,
 *    every edge index in [0, joints), the lambdas finite and >= 0, eps > 0 and t * joints <= 4608 (what one workgroup stages in LDS;
 *    T 256 at J 17 fits). */
int r50_op_geo_pose_loss_grad(const float* y, const float* gt3d, const float* gt2d, const float* K, int b, int t, int s0, int joints,
                              const int* edges_host, int n_edges, float lambda_2d, float lambda_vel, float lambda_bone, float eps,
                              float term_scale, float loss_scale, float* dy, double* part, float* out8, void* stream);

/* Forecast baselines: the nearest-neighbour search over 16-bit rows and the three trivial predictors.
 *  r50_op_row_norm2: x (n, d) 16-bit rows (et 0 = bf16, 1 = fp16) -> out (n) fp32 = |x_i|^2, summed in fp64 in a fixed order (one wave
 *    per row) and rounded once.  Needs n >= 1, d a positive multiple of 8, x 16-byte aligned, no null pointer.
 *  r50_op_nn_search: for each of the nq rows of q (nq, d) the k rows of x (n, d) with the smallest score
 *        s(q, x) = x_norm2[x] - 2 (q . x),
 *    the dot product on v_mfma_f32_16x16x32_{f16,bf16} with fp32 accumulation, K in ascending steps of 32 into one accumulator: the
 *    score of a pair depends on the two rows' values (and x_norm2[x]) alone, not on the row's position in x, on nq or on the grid.  The
 *    order is ascending by (s, index), the smaller index first at equal s: strict and total.  idx_out (nq, k) int32 and dist2_out
 *    (nq, k) fp32 = max(0, |q|^2 + s), |q|^2 as r50_op_row_norm2 computes it, are WRITTEN.  Needs nq >= 1, 1 <= k <= 8, k <= n <= 2^30,
 *    d % 32 == 0, 32 <= d <= 2048, q and x 16-byte aligned (the workspace 4-byte: fp32 scores and int32 indices), no null pointer,
 *    workspace_bytes >= r50_op_nn_search_workspace of the same
 *    nq, n, k; all checked before any launch (a refused call touches nothing).  Inputs are taken to be finite.  Per 256 queries two
 *    launches on stream: a persistent kernel sized by the CU budget (the "cu_cap" option) whose workgroups walk database chunks of 32
 *    rows (16 above d = 1024) staged once into LDS by LDS-DMA and keep a running top-k per query, then one wave per query merging the
 *    workgroups' lists.  No distance matrix is stored.  No atomics; the order being total, the result is the same bits on every run and
 *    under every CU budget.
 *  r50_op_nn_search_workspace: the bytes of device scratch the search needs (0 for arguments the search would refuse).
 *  r50_op_baseline_forecasts: a1, a0 (b, joints, 3) fp32 = the poses at the last and second-to-last observed frame; nn_row (b, k) int32
 *    device values, rows of dbj (n_db, t_db, joints, 3) fp32.  Any of three (b, pred_len, joints, 3) fp32 outputs is WRITTEN, NULL = not
 *    wanted, for h = 0 .. pred_len-1:
 *        const_pose[b,h] = a1[b]
 *        const_vel[b,h]  = fma(h + 1, a1[b] - a0[b], a1[b])                                    (one subtraction, one fma per coordinate)
 *        nn[b,h]         = a1[b,root] + (sum_i (dbj[nn_row[b,i], input_len + h] - dbj[nn_row[b,i], input_len - 1, root])) / k
 *    the sum over i = 0 .. k-1 left to right in fp32, one correctly rounded division.  Needs b, pred_len, input_len >= 1, 1 <= joints
 *    <= 64, 0 <= root < joints, a1 and at least one output; a0 with const_vel; with nn: nn_row, dbj, 1 <= k <= 8, n_db >= 1 and
 *    input_len + pred_len <= t_db; checked before any launch.  The kernel TRUSTS nn_row: the caller guarantees every value lies in
 *    [0, n_db).  One launch, gather form, no atomics. */
int r50_op_row_norm2(const void* R50_ALIGNED(16) x, int n, int d, int et, float* out, void* stream);
size_t r50_op_nn_search_workspace(int nq, int n, int k);
int r50_op_nn_search(const void* R50_ALIGNED(16) q, int nq, const void* R50_ALIGNED(16) x, int n, int d, int et, const float* x_norm2, int k, int* idx_out, float* dist2_out,
                     void* R50_ALIGNED(4) workspace, size_t workspace_bytes, void* stream);
int r50_op_baseline_forecasts(const float* a1, const float* a0, const int* nn_row, const float* dbj, int64_t n_db, int b, int k, int t_db,
                              int joints, int root, int input_len, int pred_len, float* const_pose, float* const_vel, float* nn, void* stream);

/* AdaptiveAvgPool2d((1,1)) + flatten(1): (n,hw,c) bf16 -> (n,c) fp32; c % 8 == 0.
 * Size limits: n*(c/8) + 255 < 2^31 -- one thread per image and 8 channels, numbered in an int over a grid rounded up to 256 threads -- and
 * n*hw*c*2 < 2^63 (the row offsets are 64-bit); run across 2^31 input elements and 2^32 input bytes ("Size limits"). */
int r50_op_avgpool(const void* R50_ALIGNED(16) x_nhwc_bf16, int n, int hw, int c, float* R50_ALIGNED(16) y_f32, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* R50_H_ */
