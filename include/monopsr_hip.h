/*
 * monopsr_hip.h -- C ABI of libmonopsr_hip.so: MonoPSR's per-instance hot path on MI355X (gfx950).
 *
 * This is the drop-in boundary.  Every entry point is `extern "C"`, takes plain device pointers and sizes,
 * an explicit HIP stream (passed as void* so this header needs no HIP include), returns an int status
 * (MPSR_OK == 0) and never allocates, frees or synchronises.  Outputs and scratch are caller-allocated; the
 * *_bytes / *_floats helpers say how much.  All tensors are contiguous; floats are fp32, indices int32,
 * images/activations NHWC.
 *
 * Threads: every entry point may be called from any number of threads at once (on different streams, with different
 * scratch); the library keeps no per-call state and the last-error string is thread-local.  The contraction arithmetic
 * and the Winograd policy are OPTIONS OF A CALL since ABI 5 (mpsr_net_opts.math / .winograd_policy, mpsr_conv_opts):
 * they hold for the duration of that entry point on the calling thread only, so concurrent callers with different
 * options do not see each other (the reference's launchers are stateless: tf_nndistance.cpp:168).  mpsr_set_conv_math /
 * mpsr_set_winograd_policy set the process-wide DEFAULTS that calls without options inherit -- atomics read at every
 * launch: change them before starting work, not while another thread is inside an entry point that relies on them.
 *
 * Each declaration cites the reference interface it replaces (paths under /root/reference/src).
 * The first five keep the argument order of the reference's launcher functions so the reference's TF op
 * shells (tf_nndistance.cpp:168,208 / tf_approxmatch.cpp:141-143) could bind to them with the stream appended;
 * INTEGRATION.md shows that binding and the ctypes one used by monopsr_amd.
 */
#ifndef MONOPSR_HIP_H
#define MONOPSR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void *mpsr_stream_t; /* a hipStream_t; NULL = the null stream */
typedef void *mpsr_event_t;  /* a hipEvent_t created by the caller */

enum {
    MPSR_OK = 0,
    MPSR_ERR_INVALID_ARG = 1, /* shape / pointer check failed (the reference raises errors::InvalidArgument) */
    MPSR_ERR_HIP = 2,         /* a HIP runtime call or kernel launch failed */
    MPSR_ERR_WORKSPACE = 3,   /* caller-provided scratch is too small */
    MPSR_ERR_UNSUPPORTED = 4  /* configuration outside what the kernels implement */
};

/* Human-readable description of the last non-OK status returned on the calling thread ("" if none). */
const char *mpsr_last_error(void);
/* ABI version, bumped on any signature change. */
int mpsr_abi_version(void);
/* CRC-32C (Castagnoli) of n bytes of HOST memory, continuing from `crc` (0 to start).  The checksum TensorFlow's
 * checkpoint files carry (tensor_bundle block trailers and tensor payloads); used by core/tf_checkpoint.py, which
 * replaces the tf.train.Saver restore of core/checkpoint_utils.py:64-117. */
uint32_t mpsr_crc32c(uint32_t crc, const void *data, size_t n);

/* ------------------------------------------------------------------------------------------------ Chamfer */

/* Replaces NmDistanceKernelLauncher (tf_ops/nn_distance/tf_nndistance.cpp:168, tf_nndistance_g.cu:128-131),
 * i.e. op NnDistance (tf_nndistance.cpp:3-9).  xyz1 (b,n,3), xyz2 (b,m,3) -> dist1 (b,n), idx1 (b,n),
 * dist2 (b,m), idx2 (b,m).  Squared distances; ties resolve to the lowest index; bit-exact with the
 * reference's CPU kernel (tf_nndistance.cpp:21-43).  b, n or m == 0 is a no-op. */
int mpsr_nn_distance_fwd(int b, int n, const float *xyz1, int m, const float *xyz2,
                         float *dist1, int *idx1, float *dist2, int *idx2, mpsr_stream_t stream);

/* Replaces NmDistanceGradKernelLauncher (tf_nndistance.cpp:208, tf_nndistance_g.cu:152-157), op
 * NnDistanceGrad (tf_nndistance.cpp:10-18).  Overwrites grad_xyz1 (b,n,3) and grad_xyz2 (b,m,3) (no
 * pre-zeroing needed).  idx values must lie in [0,m) / [0,n). */
int mpsr_nn_distance_bwd(int b, int n, const float *xyz1, int m, const float *xyz2,
                         const float *grad_dist1, const int *idx1, const float *grad_dist2, const int *idx2,
                         float *grad_xyz1, float *grad_xyz2, mpsr_stream_t stream);

/* ------------------------------------------------------------------------------------------------ EMD */

/* The reference has TWO implementations of the matching, and they differ numerically: its device kernel
 * (tf_approxmatch_g.cu:1-179: 10 annealing levels, fp32 state, match laid out (b,m,n) as tf_approxmatch.py:15-23
 * documents) and its CPU kernel (tf_approxmatch.cpp:23-84, the path BASELINE config 1 runs: 11 levels, double state,
 * the receiver capacity reduced by what was actually taken, match laid out (b,n,m)).  MPSR_EMD_DEVICE is the default
 * and the fast path; MPSR_EMD_HOST reproduces the CPU kernel's arithmetic on the GPU (fp64 state, libm-grade expf) so
 * that outputs can be compared with a TF1-CPU run; a few times slower. */
enum { MPSR_EMD_DEVICE = 0, MPSR_EMD_HOST = 1 };

/* Scratch floats behind `temp` for the full-speed path of the given semantics: per cloud (n+m) * (1 + levels) state
 * words (fp32, or fp64 for MPSR_EMD_HOST) -- the ratios of every level are kept so that match is written exactly once
 * (or never, mpsr_emd_loss).  mpsr_approx_match_temp_floats(b,n,m) == mpsr_emd_temp_floats(b,n,m,MPSR_EMD_DEVICE). */
size_t mpsr_emd_temp_floats(int b, int n, int m, int semantics);
size_t mpsr_approx_match_temp_floats(int b, int n, int m);

/* Replaces approxmatchLauncher (tf_approxmatch.cpp:141, tf_approxmatch_g.cu:1-182), op ApproxMatch
 * (tf_approxmatch.cpp:7-10): the launcher's arguments, then the size of `temp` in floats and the stream.
 * xyz1 (b,n,3), xyz2 (b,m,3) -> match (b,m,n), device-kernel semantics.
 *   temp_floats >= mpsr_approx_match_temp_floats(b,n,m): fast path (match written once);
 *   temp_floats >= b*(n+m)*2, what the reference's op shell allocates (tf_approxmatch.cpp:168): same result bit for
 *     bit.  The per-level state then lives in the tail of each cloud's own block of `match` until those rows are
 *     written last (same passes, same single write of match: as fast as the fast path); clouds too small or too
 *     ragged for that (n*m < 11*(n+m)+n, or more than 64 rows of state) accumulate match level by level as the
 *     reference does.  `match` must not be read by anyone else while the call runs (it never could be);
 *   less: MPSR_ERR_WORKSPACE, nothing is written. */
int mpsr_approx_match(int b, int n, int m, const float *xyz1, const float *xyz2, float *match, float *temp,
                      size_t temp_floats, mpsr_stream_t stream);

/* The same with the semantics chosen.  MPSR_EMD_HOST: match is (b,n,m) like the CPU kernel's output, temp must hold
 * mpsr_emd_temp_floats(b,n,m,MPSR_EMD_HOST) floats and be 8-byte aligned.  (mpsr_match_cost / mpsr_match_cost_grad
 * take a (b,n,m) match when called with the clouds swapped: cost(b, m, n, xyz2, xyz1, match), and
 * grad(b, m, n, xyz2, xyz1, match, grad2, grad1).) */
int mpsr_approx_match_ex(int b, int n, int m, const float *xyz1, const float *xyz2, float *match, float *temp,
                         size_t temp_floats, int semantics, mpsr_stream_t stream);

/* EarthMoversDistance (losses_custom.py:135-165: approx_match -> match_cost, gradient by MatchCostGrad with match
 * held constant) in one call that never materialises match: cost (b), grad1 = d cost / d xyz1 (b,n,3),
 * grad2 (b,m,3).  Every match entry is recomputed from the per-level ratios where it is consumed; results equal
 * mpsr_approx_match + mpsr_match_cost + mpsr_match_cost_grad to fp32 summation order.  grad1 / grad2 may be NULL
 * (cost only: the metric of monopsr_model.py:1143-1149).  temp: mpsr_emd_temp_floats(b,n,m,semantics) floats, or --
 * ABI 6 -- mpsr_emd_loss_temp_floats(b,n,m,semantics): with that much scratch (the state + both clouds re-ordered +
 * their permutations: b*(n+m)*4 floats more; device semantics, clouds of up to 4096 points) the call CAN cull levels:
 * sort both clouds into Morton order and leave out, chunk of 32 points by chunk, the pairs whose exponential
 * exp(level * d^2) is exactly zero in fp32 at the four steepest levels (-16384 .. -256: d beyond 0.08 .. 0.64) -- the
 * reference's kernels evaluate every pair at every level (tf_approxmatch_g.cu:21-160).  What is skipped is exactly zero
 * (bit-identical to the unculled evaluation of the sorted clouds), but the sums run in the order of the SORTED clouds,
 * and the annealing's clamps amplify that rounding difference: isolated gradient elements move by up to ~1e-3 of the
 * largest against the evaluation in the caller's order.  The form is therefore OFF unless switched on
 * (mpsr_debug_set_emd_cull(1): -4 .. -8 % of the call at 256 x 2048^2, slower below ~64 clouds); by default the call
 * ignores the extra scratch.  Gradients come back in the caller's point order either way. */
size_t mpsr_emd_loss_temp_floats(int b, int n, int m, int semantics);
int mpsr_emd_loss(int b, int n, int m, const float *xyz1, const float *xyz2, float *cost, float *grad1, float *grad2,
                  float *temp, size_t temp_floats, int semantics, mpsr_stream_t stream);

/* Replaces matchcostLauncher (tf_approxmatch.cpp:142, tf_approxmatch_g.cu:183-228), op MatchCost.
 * -> out (b). */
int mpsr_match_cost(int b, int n, int m, const float *xyz1, const float *xyz2, const float *match, float *out,
                    mpsr_stream_t stream);

/* Replaces matchcostgradLauncher (tf_approxmatch.cpp:143, tf_approxmatch_g.cu:229-295), op MatchCostGrad.
 * -> grad1 (b,n,3), grad2 (b,m,3); both fully overwritten. */
int mpsr_match_cost_grad(int b, int n, int m, const float *xyz1, const float *xyz2, const float *match,
                         float *grad1, float *grad2, mpsr_stream_t stream);

/* ------------------------------------------------------------------------------------------------ image ops */

/* tf.image.crop_and_resize (bilinear, extrapolation_value) as called at monopsr_model.py:222-226 and
 * net_builder.py:54-59.  image (nimg,H,W,C), boxes (nb,4) = [y1,x1,y2,x2] normalised, box_ind (nb) or NULL
 * (= all 0) -> out (nb,ch,cw,C). */
int mpsr_crop_and_resize(const float *image, int nimg, int H, int W, int C, const float *boxes,
                         const int *box_ind, int nb, int ch, int cw, float extrapolation_value, float *out,
                         mpsr_stream_t stream);

/* tf.image.resize_bilinear (TF-1.8 legacy kernel, no half-pixel centres) as called at monopsr_model.py:228-233,
 * net_builder.py:72-83 and img_preprocessor.py:32.  in (B,H,W,C) -> out (B,OH,OW,C). */
int mpsr_resize_bilinear(const float *in, int B, int H, int W, int C, int OH, int OW, int align_corners,
                         float *out, mpsr_stream_t stream);

/* slim.max_pool2d: window k, stride s, padding SAME (pad_same=1, TF pads bottom/right first) or VALID.
 * resnet_v1.py:235 (3x3/2 SAME), net_builder.py:60,68 (2x2/2 VALID). */
int mpsr_max_pool(const float *in, int B, int H, int W, int C, int k, int s, int pad_same, float *out,
                  mpsr_stream_t stream);

/* ------------------------------------------------------------------------------------------------ conv / FC */

/* One stride-1 SAME convolution (optionally atrous) or fully-connected layer as an fp32-MFMA implicit GEMM with
 * a fused epilogue: y = act(conv(x, w) + bias + residual).  Serves every slim.conv2d / slim.fully_connected on
 * the path (resnet_v1.py:116-127, resnet_utils.py:112, net_builder.py:67,77,85, monopsr_output_builder.py:101,
 * 140,166,253,...) with BatchNorm folded into w/bias by the caller.
 *   x        (B,H,W,C) NHWC, C % 4 == 0, 16-byte aligned
 *   w        (N, KH*KW*C) row-major: w[n][(ky*KW+kx)*C + c]  (the TF HWIO tensor transposed to O,HWI)
 *   bias     (N) or NULL;  residual (B,H,W,N) or NULL;  relu 0/1
 *   y        (B,H,W,N)
 *   split_k  >= 1: one output tile per workgroup; when > 1 the K loop is cut into split_k slices, `ws` must hold
 *            split_k*B*H*W*N floats (partial sums, reduced by a second kernel).
 *            0: the library schedules the launch itself -- stream-K (persistent workgroups that each take the same
 *            number of K steps of the launch's tile sequence; partial tiles meet in `ws`) when `ws` holds
 *            mpsr_conv2d_scratch_floats(B,H,W,N) floats, otherwise as split_k = 1.  Results are deterministic for
 *            a given shape and device, and equal to split_k = 1 up to fp32 summation order on the split tiles.
 *            With split_k = 0 and that scratch, large dense 3x3 layers (dilation 1, no residual, even H and W,
 *            C % 16 == 0, C and N >= 64, B*H*W >= 65536: the map decoder) run as Winograd F(2x2,3x3) -- 16
 *            products per 2x2 output tile where the direct form has 36; fp32 results agree with the direct form to
 *            ~1e-6 relative (tests/test_net_gpu.py checks 1e-5 against fp64).
 * A fully-connected layer is H=W=KH=KW=1.
 * mpsr_conv2d_plan reports, for a layer left to the library (split_k = 0, scratch given), which kernel serves it
 * (*kind: 0 implicit GEMM, 1 Winograd F(2x2,3x3), 2 direct narrow-N kernel, 3 Winograd F(4x4,3x3), 4 Winograd
 * F(3x3,3x3) -- or its sixteen-product form where a sub-grid is one zero-padded tile -- on the sub-grids of an atrous layer, 5 persistent pointwise kernel, 6 few-row fully-connected kernel) and the multiply-add FLOPs that kernel issues --
 * for throughput accounting (bench.py's roofline.executed), not needed to run anything. */
size_t mpsr_conv2d_scratch_floats(int B, int H, int W, int N);
int mpsr_conv2d_plan(int B, int H, int W, int C, int N, int KH, int KW, int dilation, int *kind,
                     double *executed_flops);
int mpsr_conv2d_nhwc_f32(const float *x, int B, int H, int W, int C, const float *w, const float *bias,
                         const float *residual, float *y, int N, int KH, int KW, int dilation, int relu,
                         int split_k, float *ws, size_t ws_floats, mpsr_stream_t stream);

/* Options of ONE call (ABI 5).  The reference's launchers carry no state (tf_nndistance.cpp:168); here the
 * arithmetic mode and the Winograd policy have process-wide defaults (mpsr_set_conv_math / mpsr_set_winograd_policy
 * below) and every entry point that takes options can override them for the duration of the call -- calls on different
 * host threads with different options do not see each other (tests/test_threads_gpu.py).  A zero-initialised struct
 * inherits the defaults. */
enum { MPSR_CALL_MATH_INHERIT = 0, MPSR_CALL_MATH_FP32 = 1, MPSR_CALL_MATH_BF16X3 = 2 };
enum { MPSR_CALL_WINOGRAD_INHERIT = 0, MPSR_CALL_WINOGRAD_AUTO = 1, MPSR_CALL_WINOGRAD_OFF = 2,
       MPSR_CALL_WINOGRAD_ACCURATE = 3 /* ABI 6 */ };
typedef struct mpsr_conv_opts {
    int32_t math;            /* MPSR_CALL_MATH_* */
    int32_t winograd_policy; /* MPSR_CALL_WINOGRAD_* */
} mpsr_conv_opts;
int mpsr_conv2d_nhwc_f32_ex(const float *x, int B, int H, int W, int C, const float *w, const float *bias,
                            const float *residual, float *y, int N, int KH, int KW, int dilation, int relu,
                            int split_k, float *ws, size_t ws_floats, const mpsr_conv_opts *opts, mpsr_stream_t stream);

/* Arithmetic of every contraction mpsr_conv2d_nhwc_f32 and the network entry points run (process-wide DEFAULT;
 * per call: mpsr_conv_opts / mpsr_net_opts).
 *   MPSR_MATH_FP32   (default) exact fp32 products on v_mfma_f32_32x32x2_f32: what every parity and benchmark
 *                    number of this library refers to unless it says otherwise.
 *   MPSR_MATH_BF16X3 opt-in fast mode: operands split into hi + lo bfloat16 halves on the fly, each product evaluated
 *                    as hi*hi + hi*lo + lo*hi on v_mfma_f32_32x32x16_bf16 with fp32 accumulation (~2^-16 relative
 *                    error per product; inputs, outputs and weights stay fp32 in memory).
 * The reference has no such switch (TF-1.8 convolutions are fp32); the path's drift budget is 1e-3 (BASELINE.json). */
enum { MPSR_MATH_FP32 = 0, MPSR_MATH_BF16X3 = 1 };
int mpsr_set_conv_math(int mode);
int mpsr_get_conv_math(void);

/* Whether 3x3 layers may run in a Winograd transform domain (process-wide DEFAULT, like the arithmetic above; per call:
 * mpsr_conv_opts / mpsr_net_opts).
 *   MPSR_WINOGRAD_AUTO (default) block3's atrous layers (one zero-padded 3x3 tile per pixel sub-grid) in sixteen
 *                      products per tile, F(3x3,3x3) on the tiles-with-halos of blocks 1-2, F(4x4,3x3) / F(2x2,3x3) on
 *                      the dense decoder layers wherever they are faster.  Error against float64 of the tensor's
 *                      SCALE: 3e-7 / 3e-6 / 1.5e-5 / 1e-6 (a direct fp32 convolution: 2.5e-7 .. 5e-7) -- far inside the
 *                      path's 1e-3 budget.  The transforms mix the values of a whole input patch, so a SMALL output
 *                      next to a very large activation carries an error relative to the large one: on maps with 1 % of
 *                      the entries 1000x the rest, elements down to 1e-3 of the tensor's maximum were measured
 *                      2e-3 .. 4e-3 off relative to THEMSELVES under F(4x4,3x3), 0.5e-3 .. 2e-3 under F(3x3,3x3) with
 *                      halos, 2e-4 in the sixteen-product form (the direct kernels 1e-4;
 *                      tests/test_hostile_inputs_gpu.py).  The decoder end to end on such features (100x outliers):
 *                      1.2e-3, where fp32 arithmetic without any Winograd kernel measures 8.6e-4.
 *   MPSR_WINOGRAD_OFF  direct / implicit-GEMM kernels everywhere (the upsampled convolutions keep their exact tap
 *                      GEMM): element-wise 5e-5 .. 1e-4 on the same inputs, at 1.33x the step time (17.8 vs 13.4 ms:
 *                      bench.py's `winograd_off_mode` object times it and measures both policies' errors).  For callers whose
 *                      activations are heavy-tailed AND who read small outputs individually.
 *   MPSR_WINOGRAD_ACCURATE (r06) only the transform-domain forms whose ELEMENT-WISE error on such maps stays inside
 *                      1e-3: the sixteen-product form for block3's atrous layers (2e-4) and F(2x2,3x3) for the dense
 *                      decoder layers (transform constants 1 and 1/2); F(4x4,3x3) and the F(3x3,3x3) halo tiles are not
 *                      used (their layers take F(2x2,3x3) / the direct kernels).  Between the two above in speed
 *                      (bench.py's `winograd_accurate_mode`). */
enum { MPSR_WINOGRAD_AUTO = 0, MPSR_WINOGRAD_OFF = 1, MPSR_WINOGRAD_ACCURATE = 2 };
int mpsr_set_winograd_policy(int policy);
int mpsr_get_winograd_policy(void);

/* tf.image.resize_bilinear (align_corners as given) followed by a 3x3 SAME slim.conv2d, as the map decoder applies
 * them (monopsr/builders/net_builder.py:72-77, :81-85), WITHOUT forming the upsampled map: a 1x1 GEMM of the source
 * map with 9 N outputs (channel mixing commutes with the per-channel upsampling) + a 9-tap x 4-corner gather
 * (csrc/upconv.hip).  x (B,h,w,C) -> y (B,OH,OW,N) NHWC; weights (N, 9 C) as for mpsr_conv2d_nhwc_f32.  Needs
 * N % 128 == 0, C % 64 == 0, C >= 128 (MPSR_ERR_UNSUPPORTED otherwise: use mpsr_resize_bilinear + mpsr_conv2d_nhwc_f32)
 * and mpsr_conv3x3_upsampled_scratch_floats() floats of scratch.  fp32 arithmetic whatever mpsr_set_conv_math says. */
size_t mpsr_conv3x3_upsampled_scratch_floats(int B, int h, int w, int C, int N);
int mpsr_conv3x3_upsampled_f32(const float *x, int B, int h, int w, int C, int OH, int OW, int align_corners,
                               const float *weights, const float *bias, int relu, float *y, int N, float *ws,
                               size_t ws_floats, mpsr_stream_t stream);
/* 0: the shape is outside what mpsr_conv3x3_upsampled_f32 takes; 1: forward only; 2: forward and backward. */
int mpsr_conv3x3_upsampled_applies(int B, int h, int w, int C, int OH, int OW, int N, int align_corners);
/* Its backward for training (TF autodiff of the two operators in the reference): dy (B,OH,OW,N) = gradient at the
 * convolution's output BEFORE bias / activation.  dw (N, 9 C) += weight gradient (accumulated, like
 * mpsr_conv2d_wgrad_f32; the bias gradient is mpsr_bias_grad of dy); dx (B,h,w,C) = data gradient, or NULL.  Everything
 * happens at the SOURCE resolution: dz = the transposed gather of dy, then a 1x1 weight gradient and a 1x1 GEMM with
 * K = 9 N -- in place of the resize gradient + the 3x3 data and weight gradients on the upsampled map.  Deterministic
 * except for the weight gradient's pixel slices (fp32 atomics, as mpsr_conv2d_wgrad_f32). */
size_t mpsr_conv3x3_upsampled_bwd_scratch_floats(int B, int h, int w, int C, int N);
int mpsr_conv3x3_upsampled_bwd_f32(const float *x, const float *dy, int B, int h, int w, int C, int OH, int OW,
                                   int align_corners, const float *weights, int N, float *dw, float *dx, float *ws,
                                   size_t ws_floats, mpsr_stream_t stream);

/* Explicit im2col for the ResNet root: explicit zero pad 3 + 7x7 stride-2 VALID (resnet_utils.py:115-122 via
 * resnet_v1.py:234).  x (B,H,W,3) -> cols (B*OH*OW, kpad) with OH=(H+6-7)/2+1; column (ky*7+kx)*3+c, columns
 * 147..kpad-1 zero.  kpad % 32 == 0, kpad >= 147. */
int mpsr_im2col_root(const float *x, int B, int H, int W, float *cols, int kpad, mpsr_stream_t stream);

/* ------------------------------------------------------------------------------------------------ backward */
/* The reference gets gradients from TensorFlow autodiff (core/trainer.py:71-81, builders/optimizer_builder.py:61-80);
 * these entry points are what a training step of the instance path needs beyond the forward kernels. */

/* dW[n][(ky*KW+kx)*C + c] += sum over pixels of dy[pixel][n] * x[pixel + tap][c] (same geometry as
 * mpsr_conv2d_nhwc_f32).  x (B,H,W,C), dy (B,H,W,N), dw (N, KH*KW*C) must be zeroed by the caller (partial sums
 * from pixel slices are combined with fp32 atomics).  C % 4 == 0, N % 4 == 0.
 * db (N) or NULL: the bias gradient db[n] += sum over pixels of dy[pixel][n] rides along (column sums of the dy
 * tiles the kernel stages anyway; also pre-zeroed by the caller). */
int mpsr_conv2d_wgrad_f32(const float *x, const float *dy, int B, int H, int W, int C, int N, int KH, int KW,
                          int dilation, float *dw, float *db, mpsr_stream_t stream);
/* The same with caller scratch: `ws` of at least mpsr_conv2d_wgrad_scratch_floats(...) floats (0 when the layer does
 * not use any) lets the big dense 3x3 layers (the map decoder: stride 1, no dilation, H and W multiples of 4, C and N
 * multiples of 32 and at least 128, B*H*W >= 131072) run in the Winograd F(4x4,3x3) domain -- 36 products per channel pair and 4x4
 * block where the direct weight gradient has 144; results agree with mpsr_conv2d_wgrad_f32 to ~1e-4 of the
 * gradient's scale.  ws = NULL or too small: exactly mpsr_conv2d_wgrad_f32.
 * Run-to-run reproducibility: BOTH forms combine the partial sums of their pixel / tile slices with fp32 atomics, so a
 * weight gradient's last bits depend on the order in which workgroups arrive (relative spread ~1e-7 direct, ~1e-6 in
 * the Winograd domain, where the transformed sums are larger); forward results and data gradients are deterministic. */
size_t mpsr_conv2d_wgrad_scratch_floats(int B, int H, int W, int C, int N, int KH, int KW, int dilation);
int mpsr_conv2d_wgrad_ws_f32(const float *x, const float *dy, int B, int H, int W, int C, int N, int KH, int KW,
                             int dilation, float *dw, float *db, float *ws, size_t ws_floats, mpsr_stream_t stream);
/* ABI 13: which kernel mpsr_conv2d_wgrad_ws_f32 launches for a shape when it is given ws_floats floats of scratch -- pure
 * host code with the argument checks of mpsr_conv2d_wgrad_f32, reading the same predicates and slice arithmetic as the
 * launchers.  kind: 0 = the general kernel (conv_wgrad_kernel), 1 = the 1x1 layers' direct-operand kernel
 * (pw_wgrad_direct_kernel), 2 = the thin head kernel (N = 4; it also wants dy on a 16-byte boundary, which the plan
 * assumes), 3 = the F(4x4,3x3) domain (only with ws_floats >= mpsr_conv2d_wgrad_scratch_floats), 4 = the F(3x3,3x3)
 * domain.  For kinds 3 and 4 the tile sum is cut into `nslices` slices of `steps` K steps (8 tiles each for kind 3, 4
 * for kind 4; steps is even) over `tiles` tiles: the last slice holds tiles - (nslices - 1) * steps * 8 (or 4) live
 * tiles, the rest of it is zero-filled.  Other kinds: tiles = steps = nslices = 0.  Any out-pointer may be NULL. */
int mpsr_conv2d_wgrad_plan(int B, int H, int W, int C, int N, int KH, int KW, int dilation, size_t ws_floats, int *kind,
                           int *tiles, int *steps, int *nslices);

/* Weight re-layout for the data gradient: wd[c][((KH*KW-1-t)*N) + n] = w[n][t*C + c].  Then
 * dx = mpsr_conv2d_nhwc_f32(dy, ..., w = wd, N := C, C := N) with the same KH, KW, dilation. */
int mpsr_conv2d_dgrad_pack(const float *w, int N, int KH, int KW, int C, float *wd, mpsr_stream_t stream);

/* The re-layout of ALL the layers of a training step in one launch (the reference's step differentiates every layer of
 * the graph in one session.run: core/trainer.py:76-81, builders/optimizer_builder.py:61-80; here the weights only
 * change in the optimizer step, so their data-gradient layouts are made once per step, not once per layer launch).
 * A job = one layer: w (N, T = KH*KW, C) -> wd (C, T, Nd) with Nd >= N (a filter padded to Nd output channels: rows
 * N..Nd-1 read as zero).  The caller describes the jobs once (`chunk0` is filled in by the library), builds the table
 * on the host, copies its mpsr_dgrad_pack_table_bytes() bytes to device memory and from then on issues
 * mpsr_conv2d_dgrad_pack_batch(table_dev, n_chunks) whenever the weights changed.  Pointers inside the table are
 * device pointers and must stay valid; the table holds no other state. */
typedef struct mpsr_pack_job {
    const float *w;
    float *wd;
    int32_t N, Nd, T, C;
    int64_t chunk0;
} mpsr_pack_job;
size_t mpsr_dgrad_pack_table_bytes(const mpsr_pack_job *jobs, int n_jobs); /* 0 = bad jobs */
int mpsr_dgrad_pack_table_build(const mpsr_pack_job *jobs, int n_jobs, void *table_host, long long *n_chunks);
int mpsr_conv2d_dgrad_pack_batch(const void *table_dev, long long n_chunks, mpsr_stream_t stream);

/* Fused activation + bias gradient in one pass over dy (M,N): g = (y > 0 ? dy : 0) when y != NULL else dy;
 * dx = g when dx != NULL (may alias dy); db[n] += sum_m g[m][n] when db != NULL (zeroed by the caller). */
int mpsr_act_bias_grad(const float *dy, const float *y, float *dx, float *db, long long M, int N,
                       mpsr_stream_t stream);

/* db[n] += sum_m dy[m][n]; db zeroed by the caller. */
int mpsr_bias_grad(const float *dy, long long M, int N, float *db, mpsr_stream_t stream);

/* dx = dy where y > 0 else 0 (y = post-activation output of the layer).  dx may alias dy. */
int mpsr_relu_grad(const float *dy, const float *y, float *dx, long long total, mpsr_stream_t stream);

/* The ReLU mask of a tensor as bits, and a 1x1 data gradient that leaves through it (training: a bottleneck unit's
 * input gradient, TF autodiff of resnet_v1.py:104-135, without the elementwise ReLU-gradient pass over it).
 * Layout: bits[(m >> 5) * N + n], bit b <-> row m = 32 (m >> 5) + (b & 3) + 8 ((b >> 2) & 3) + 4 (b >> 4) -- the
 * accumulator layout of the 32x32 MFMA, so that a convolution can write the words from its epilogue;
 * mpsr_relu_bitmask_words(M, N) = ceil(M / 32) * N words, 16-byte aligned; N % 4 == 0.
 * mpsr_relu_bitmask: the words of y (M,N): bit = (y[m][n] > 0), rows >= M zero.
 * mpsr_conv1x1_relu_bitmask_f32: y = act(x w^T + bias + residual) on the persistent pointwise kernel AND the words
 * of y in the same launch (bits of rows >= M unspecified); y is bit-identical to mpsr_conv2d_nhwc_f32's.
 * mpsr_conv1x1_masked_f32: y[m][n] = bit(m, n) ? sum_k x[m][k] w[n][k] + bias[n] + residual[m][n] : 0 (bias,
 * residual may be NULL); kept elements are bit-identical to the unmasked launch.
 * mpsr_conv1x1_masked_applies says whether the shape (and the arithmetic mode: fp32 only) is taken by the last two --
 * otherwise MPSR_ERR_UNSUPPORTED and the caller runs mpsr_conv2d_nhwc_f32 (+ mpsr_relu_grad). */
/* y = conv(x, w) (no bias, as scheduled by the library: split_k = 0 of mpsr_conv2d_nhwc_f32, same scratch) where
 * mask > 0 and zero elsewhere; mask (B,H,W,N) = the post-ReLU tensor this data gradient belongs to.  The F(3x3,3x3)
 * atrous kernel (block3's conv2) applies it in its epilogue, other shapes run mpsr_relu_grad in place afterwards. */
int mpsr_conv2d_relu_masked_f32(const float *x, int B, int H, int W, int C, const float *w, const float *mask, float *y,
                                int N, int KH, int KW, int dilation, float *ws, size_t ws_floats, mpsr_stream_t stream);
long long mpsr_relu_bitmask_words(long long M, int N);
int mpsr_relu_bitmask(const float *y, long long M, int N, unsigned *bits, mpsr_stream_t stream);
int mpsr_conv1x1_masked_applies(long long M, int K, int N);
int mpsr_conv1x1_relu_bitmask_f32(const float *x, long long M, int K, const float *w, const float *bias,
                                  const float *residual, int relu, float *y, unsigned *bits, int N, mpsr_stream_t stream);
int mpsr_conv1x1_masked_f32(const float *x, long long M, int K, const float *w, const float *bias,
                            const float *residual, const unsigned *mask, float *y, int N, mpsr_stream_t stream);

/* Gradient of mpsr_max_pool w.r.t. its input (first maximum of each window takes the gradient); dx (B,H,W,C) is
 * fully overwritten. */
int mpsr_max_pool_grad(const float *x, const float *dy, int B, int H, int W, int C, int k, int s, int pad_same,
                       float *dx, mpsr_stream_t stream);

/* Gradient of mpsr_resize_bilinear w.r.t. its input; dy (B,OH,OW,C) -> dx (B,H,W,C), fully overwritten. */
int mpsr_resize_bilinear_grad(const float *dy, int B, int H, int W, int C, int OH, int OW, int align_corners,
                              float *dx, mpsr_stream_t stream);

/* One Adam step over flat fp32 buffers (tf.train.AdamOptimizer update rule, optimizer_builder.py:61-80):
 * g' = grad*grad_scale; m = b1*m+(1-b1)*g'; v = b2*v+(1-b2)*g'^2; p -= lr*sqrt(1-b2^step)/(1-b1^step) * m/(sqrt(v)+eps). */
int mpsr_adam_step(float *param, const float *grad, float *m, float *v, long long n, float lr, float beta1,
                   float beta2, float eps, int step, float grad_scale, mpsr_stream_t stream);
/* The same update with the bias-corrected rate lr_t = lr*sqrt(1-b2^step)/(1-b1^step) read from DEVICE memory when the
 * kernel runs: a launch captured into a HIP graph (the training step replayed as one graph launch) then follows the
 * schedule -- the caller writes *lr_t_dev (stream-ordered) before each replay. */
int mpsr_adam_step_lr_dev(float *param, const float *grad, float *m, float *v, long long n, const float *lr_t_dev,
                          float beta1, float beta2, float eps, float grad_scale, mpsr_stream_t stream);

/* Gradient of mpsr_crop_and_resize w.r.t. the image (TensorFlow's CropAndResizeGradImage, reached through autodiff
 * from net_builder.py:54-59 when the full-image trunk trains).  grad_out (nb,ch,cw,C) -> grad_image (nimg,H,W,C),
 * zeroed inside and accumulated with fp32 atomics; samples that were extrapolated contribute nothing. */
int mpsr_crop_and_resize_grad(const float *grad_out, int nimg, int H, int W, int C, const float *boxes,
                              const int *box_ind, int nb, int ch, int cw, float *grad_image, mpsr_stream_t stream);

/* Training-mode batch normalisation of the map decoder (net_builder.py:76-87: slim.batch_norm with is_training,
 * statistics over (N,H,W) per channel, no scale, epsilon 1e-3, then ReLU).  z is the (M, C) convolution output,
 * M = N*H*W, C % 4 == 0, C <= 1024.  Statistics are accumulated in fp64 around the first row for conditioning:
 *   sum[c] = sum_m (z[m][c] - z[0][c]),  sumsq_shifted[c] = sum_m (z[m][c] - z[0][c])^2
 * so mean = z[0] + sum/M and the (biased) variance = sumsq_shifted/M - (sum/M)^2.
 * Alignment: every (M, C) tensor and every per-channel float vector of the entry points below that stream them (_stats,
 * _apply, _grad_sums[_z], _grad[_z]) is accessed 16 bytes at a time; a pointer that is not a multiple of 16 is refused
 * (status 1) before anything is launched.  The fp64 sums and the operands of the two _finalize calls need only their
 * natural alignment.
 * NaN: a NaN anywhere in a channel of z makes that channel's sums, mean, variance, inv_std and BOTH moving statistics
 * NaN (the variance is clamped at 0 from below only; a NaN is not clamped away); other channels are unaffected. */
int mpsr_batch_norm_stats(const float *z, long long M, int C, double *sum, double *sumsq_shifted,
                          mpsr_stream_t stream);
/* ABI 6: the per-channel arithmetic between the passes as one launch each (they were ~16 and ~4 tiny tensor operations
 * per layer and step on the host framework's side).  Forward: d = sum / M, mean = z_row0 + d (z_row0 = the first row of
 * z, the shift of the sums), var = max(sumsq_shifted / M - d^2, 0) (a NaN stays NaN) in fp64; mean and
 * inv_std = 1 / sqrt(var + eps) as floats; moving_mean = moving_mean * decay + (1 - decay) * mean and moving_variance likewise with the UNBIASED
 * variance var * M / max(M - 1, 1), as TensorFlow's fused kernel feeds its moving average (either may be NULL: not
 * updated).  Backward: dbeta += sum_g (NULL: not deposited), mean_g = sum_g / count, mean_gz = sum_gz / count (count =
 * the rows the statistics were taken over).  A caller that pools the sums over ranks does this arithmetic itself. */
int mpsr_batch_norm_finalize(const double *sum, const double *sumsq_shifted, const float *z_row0, long long M, int C,
                             float eps, float decay, float *moving_mean, float *moving_variance, float *mean,
                             float *inv_std, mpsr_stream_t stream);
int mpsr_batch_norm_grad_finalize(const double *sum_g, const double *sum_gz, double count, int C, float *dbeta,
                                  float *mean_g, float *mean_gz, mpsr_stream_t stream);
/* y = act((z - mean) * inv_std + beta); relu 0/1; mean, inv_std, beta (C). */
int mpsr_batch_norm_apply(const float *z, long long M, int C, const float *mean, const float *inv_std,
                          const float *beta, int relu, float *y, mpsr_stream_t stream);
/* Backward, pass 1: with g = dy * (y > 0) (g = dy when y == NULL) and zhat = (z - mean) * inv_std:
 * sum_g[c] = sum_m g (= the beta gradient), sum_gz[c] = sum_m g * zhat; fp64, zeroed inside. */
int mpsr_batch_norm_grad_sums(const float *dy, const float *y, const float *z, long long M, int C, const float *mean,
                              const float *inv_std, double *sum_g, double *sum_gz, mpsr_stream_t stream);
/* Backward, pass 2: dz = inv_std * (g - mean_g - zhat * mean_gz), mean_g = sum_g / M, mean_gz = sum_gz / M. */
int mpsr_batch_norm_grad(const float *dy, const float *y, const float *z, long long M, int C, const float *mean,
                         const float *inv_std, const float *mean_g, const float *mean_gz, float *dz,
                         mpsr_stream_t stream);

/* ABI 6: the same two passes for a layer with ReLU WITHOUT reading y: the mask y > 0 is rebuilt from z as
 * relu((z - mean) * inv_std + beta) > 0 with mpsr_batch_norm_apply's own fused multiply-add (the same bits), which takes
 * one of the three (four) tensor-sized streams out of each pass. */
int mpsr_batch_norm_grad_sums_z(const float *dy, const float *z, long long M, int C, const float *mean,
                                const float *inv_std, const float *beta, double *sum_g, double *sum_gz,
                                mpsr_stream_t stream);
int mpsr_batch_norm_grad_z(const float *dy, const float *z, long long M, int C, const float *mean, const float *inv_std,
                           const float *beta, const float *mean_g, const float *mean_gz, float *dz, mpsr_stream_t stream);

/* tf.clip_by_norm applied to every variable of a flat gradient buffer separately, as
 * slim.learning.create_train_op(clip_gradient_norm=1.0) does (core/trainer.py:78-81): g *= clip / max(||g||, clip).
 * The caller describes the variables once as a chunk table (device arrays): chunk i covers
 * grads[chunk_begin[i] .. +chunk_len[i]) and belongs to variable chunk_seg[i] in [0, n_segments).
 * chunk_seg ascends (a variable's chunks are consecutive).
 * sumsq: scratch of sumsq_floats >= n_segments + n_chunks floats (MPSR_ERR_WORKSPACE otherwise): the first n_segments
 * hold each variable's squared norm on return, the rest the chunks' partial sums.  ABI 6 (signature changed: sumsq_floats):
 * the norms are summed in a FIXED order -- per chunk, then over a variable's chunks -- with no atomics, so every replica of
 * a data-parallel run scales the same reduced gradient by the same bits and the replicas' parameters stay bit-identical
 * (tests/test_sharded_training_step_gpu.py; an atomic accumulation left two ranks one ulp apart after one step).
 * Any ascending table is served (tests/test_optim_gpu.py): chunk_begin needs no alignment (a chunk that does not start on
 * 16 bytes is read float by float); a chunk of length 0 is allowed and adds nothing; a segment id in [0, n_segments) with
 * no chunk gets the squared norm 0; chunks may leave gaps, and elements outside every chunk are neither read nor written.
 * The scale is applied iff norm > clip_norm, strictly: a variable with norm == clip_norm keeps its bits, and so does one
 * whose norm is NaN (a NaN among its elements) -- its gradient is left as it is.  An infinite norm over a finite
 * clip_norm scales by clip_norm / inf = 0: finite elements become +-0, the infinite ones NaN (what
 * g * clip / max(norm, clip) gives); against clip_norm = +inf it is norm == clip_norm, not scaled. */
int mpsr_clip_by_norm_segments(float *grads, const int *chunk_seg, const long long *chunk_begin,
                               const int *chunk_len, int n_chunks, float *sumsq, size_t sumsq_floats, int n_segments,
                               float clip_norm, mpsr_stream_t stream);

/* ABI 6: the tail of a training step in three launches -- per-variable tf.clip_by_norm (core/trainer.py:78-81), the Adam
 * update (builders/optimizer_builder.py:61-80) and the parameter moving average (tf.contrib.opt.MovingAverageOptimizer,
 * optimizer_builder.py:75-80) over the same chunk table: squared norms, then ONE pass that scales the gradient on its way
 * into the update (grads are left as they came), updates m / v / param and, when `shadow` is not NULL,
 * shadow += (1 - ema_decay) * (param - shadow).  Operation by operation the arithmetic of mpsr_clip_by_norm_segments ->
 * mpsr_adam_step -> that moving average; elements outside every chunk (alignment padding) are not touched.
 * clip_norm <= 0: no clipping (sumsq may be NULL).  sumsq / sumsq_floats as mpsr_clip_by_norm_segments (deterministic
 * norms).  step = 1-based Adam step (bias correction).
 * The table semantics are mpsr_clip_by_norm_segments': no alignment requirement on chunk_begin, zero-length chunks
 * allowed, a segment id with no chunk gets norm 0, norm == clip_norm is not scaled, and a NaN norm leaves the segment's
 * gradient as it is (scale 1: only the NaN elements' own param / m / v become NaN).  sumsq[0 .. n_segments) holds the
 * same bits mpsr_clip_by_norm_segments writes for the same gradients.  Outside every chunk none of param, grad, m, v and
 * shadow is read or written. */
int mpsr_clip_adam_ema_step(float *param, const float *grad, float *m, float *v, float *shadow, const int *chunk_seg,
                            const long long *chunk_begin, const int *chunk_len, int n_chunks, float *sumsq,
                            size_t sumsq_floats, int n_segments, float clip_norm, float lr, float beta1, float beta2,
                            float eps, int step, float ema_decay, mpsr_stream_t stream);

/* ------------------------------------------------------------------------- per-box geometry and map losses
 * SURVEY.md 8(f) rows 3-4.  Maps are (b, h, w, c) row-major; p = h*w points per instance. */

/* instance_utils.py:567-602 tf_inst_xyz_map_local_to_global: xyz_global = T(centroid) R_y(view_ang) xyz_local.
 * xyz_local/xyz_global (b,p,3); view_angs (b); centroids (b,3). */
int mpsr_xyz_map_local_to_global(const float *xyz_local, const float *view_angs, const float *centroids,
                                 float *xyz_global, int b, int p, mpsr_stream_t stream);

/* Its gradient: grad_local (b,p,3) = R^T grad_global, grad_centroids (b,3) = sum over points; either may be NULL. */
int mpsr_xyz_map_local_to_global_grad(const float *grad_global, const float *view_angs, float *grad_local,
                                      float *grad_centroids, int b, int p, mpsr_stream_t stream);

/* monopsr_output_builder.py:681-746 get_proj_err_maps_norm: (expected pixel-centre grid of the 2-D box - projection
 * of xyz_global by cam_p) / box [w,h], * valid_mask, clipped to [-2,2] -> proj_err_maps (b,h,w,2) (may be NULL);
 * proj_err_norm (b) = sum over the map / max(sum(valid_mask), 1).  boxes_2d (b,4) [y1,x1,y2,x2]; cam_p (12);
 * valid_mask (b,h,w). */
int mpsr_proj_err_norm(const float *xyz_global, const float *boxes_2d, const float *cam_p, const float *valid_mask,
                       float *proj_err_maps, float *proj_err_norm, int b, int h, int w, mpsr_stream_t stream);

/* d(sum_b grad_proj_err_norm[b] * proj_err_norm[b]) / d xyz_global -> grad_xyz_global (b,h,w,3), overwritten. */
int mpsr_proj_err_norm_grad(const float *grad_proj_err_norm, const float *xyz_global, const float *boxes_2d,
                            const float *cam_p, const float *valid_mask, float *grad_xyz_global, int b, int h, int w,
                            mpsr_stream_t stream);

/* Per-box cameras for the two projection-error entry points -- the boxes of several frames in one call, the convention
 * of mpsr_heads_fwd_cams: cam_p (n_cams,12); cam_index (b) int32 picks each box's matrix; NULL: every box uses the first.
 * An index outside [0, n_cams) is never dereferenced: that box's proj_err_maps / proj_err_norm / grad_xyz_global come
 * back NaN, the other boxes are not affected and no error is recorded.  A box's arithmetic is that of the single-camera
 * entry points (which are these with n_cams = 1 and a NULL index): one workgroup per box, same operation order. */
int mpsr_proj_err_norm_cams(const float *xyz_global, const float *boxes_2d, const float *cam_p, int n_cams,
                            const int *cam_index, const float *valid_mask, float *proj_err_maps, float *proj_err_norm,
                            int b, int h, int w, mpsr_stream_t stream);
int mpsr_proj_err_norm_grad_cams(const float *grad_proj_err_norm, const float *xyz_global, const float *boxes_2d,
                                 const float *cam_p, int n_cams, const int *cam_index, const float *valid_mask,
                                 float *grad_xyz_global, int b, int h, int w, mpsr_stream_t stream);

/* instance_utils.py:605-680 tf_inst_depth_map_local_to_global: depth_global (b,h,w) = depth_local + cen_z[b]
 * (+ the view-normalisation offset, linear along the ROW axis as the reference lays it out, when rotate_view).
 * depth_local is read with a stride of depth_stride floats (3 to read the z channel of an xyz map in place). */
int mpsr_depth_map_local_to_global(const float *depth_local, int depth_stride, const float *cen_z,
                                   const float *boxes_2d, const float *view_angs, const float *cam_p,
                                   float *depth_global, int b, int h, int w, int rotate_view, mpsr_stream_t stream);

/* Gradient w.r.t. cen_z (b); the gradient w.r.t. depth_local is grad_global itself. */
int mpsr_depth_map_local_to_global_grad(const float *grad_global, const float *boxes_2d, const float *view_angs,
                                        const float *cam_p, float *grad_cen_z, int b, int h, int w, int rotate_view,
                                        mpsr_stream_t stream);

/* The same two with per-box cameras (cam_p (n_cams,12), cam_index (b) or NULL, as mpsr_proj_err_norm_cams).  The
 * camera is read only when rotate_view is set; an index outside [0, n_cams) then gives NaN in that box's depth_global /
 * grad_cen_z and is never dereferenced. */
int mpsr_depth_map_local_to_global_cams(const float *depth_local, int depth_stride, const float *cen_z,
                                        const float *boxes_2d, const float *view_angs, const float *cam_p, int n_cams,
                                        const int *cam_index, float *depth_global, int b, int h, int w,
                                        int rotate_view, mpsr_stream_t stream);
int mpsr_depth_map_local_to_global_grad_cams(const float *grad_global, const float *boxes_2d, const float *view_angs,
                                             const float *cam_p, int n_cams, const int *cam_index, float *grad_cen_z,
                                             int b, int h, int w, int rotate_view, mpsr_stream_t stream);

/* Per-instance sums behind WeightedNonZeroSmoothL1LocalizationLoss (losses_custom.py:93-132, tf.losses.huber_loss
 * with Reduction.SUM_BY_NONZERO_WEIGHTS): pred/target (b,p,c), weights (b,p) broadcast over c.
 * sums[b] = sum huber(pred-target)*w; counts[b] = c * #(w != 0).  loss = sum(sums)/sum(counts) (0 if none). */
int mpsr_huber_loss_sums(const float *pred, const float *target, const float *weights, int b, int p, int c,
                         float delta, float *sums, float *counts, mpsr_stream_t stream);

/* grad (b,p,c) = scale[0] * w * clamp(pred - target, -delta, delta); scale is a DEVICE scalar (so the caller can
 * derive it from sums/counts without a host sync). */
int mpsr_huber_loss_grad(const float *pred, const float *target, const float *weights, const float *scale, int b,
                         int p, int c, float delta, float *grad, mpsr_stream_t stream);

/* mpsr_huber_loss_grad with one DEVICE scale per instance: grad (b,p,c) = scale[instance] * w * clamp(pred - target,
 * -delta, delta).  A step over several frames normalises every frame's map loss by that frame's own valid-pixel count
 * (MonoPSRModel.loss_batch): the scale of an instance is its frame's. */
int mpsr_huber_loss_grad_scales(const float *pred, const float *target, const float *weights, const float *scale,
                                int b, int p, int c, float delta, float *grad, mpsr_stream_t stream);

/* monopsr_model.py:960-1071 format_predictions (test mode; lwh offset, alpha 'dc', view_ang est, centroids xyz)
 * with instance_utils.py:988-1032 postprocess_cen_x and monopsr_output_builder.py:805-860 score_boxes, one thread
 * per box in fp64: box_3d (b,9) = [x,y,z,l,w,h,ry,score,class-1], box_2d (b,7) = [y1,x1,y2,x2,alpha,score,class-1].
 * lwh (b,3); view_angs (b); alpha_bins/alpha_regs (b,num_alpha_bins); centroids (b,3); boxes_2d (b,4);
 * scores (b); class_idx (b) int32; cam_p (12). */
int mpsr_format_boxes(const float *lwh, const float *view_angs, const float *alpha_bins, const float *alpha_regs,
                      const float *centroids, const float *boxes_2d, const float *scores, const int *class_idx,
                      const float *cam_p, int b, int num_alpha_bins, int img_h, int img_w, int centroid_middle,
                      int post_process_cen_x, float max_depth, float *box_3d, float *box_2d, mpsr_stream_t stream);

/* ------------------------------------------------------------------------------------------------ network */

/* One packed convolution / FC layer inside a weight blob (offsets in floats from the blob base). */
typedef struct mpsr_layer {
    int32_t cin, cout, kh, kw, dilation, relu;
    int64_t w_off; /* (cout, kh*kw*cin) BN-folded weights */
    int64_t b_off; /* (cout) folded bias, or -1 */
} mpsr_layer;

/* Optional arguments of the *_ex network entry points (NULL = none; zero-initialise, then set what is wanted).
 *  - filter_cache: the Winograd kernels (F(3x3,3x3) on block3's atrous layers, F(4x4,3x3) on the map decoder) multiply
 *    by TRANSFORMED filters G g G^T.  Without a cache they are recomputed from `blob` by every call (a launch or a tail
 *    job per layer).  With a caller-owned buffer of mpsr_filter_cache_floats() floats they are written there by the
 *    first call (filter_cache_valid = 0) and only read by later calls that pass filter_cache_valid != 0 -- the caller
 *    vouches that blob / layers / B / shape are the ones the cache was filled for (inference: weights never change;
 *    a training loop passes 0 or no cache).  A cache that is too small is used for the layers that fit.  Which form a
 *    layer's filters take depends on the kernel the call picks (batch size, mpsr_set_conv_math,
 *    mpsr_set_winograd_policy): pass filter_cache_tags and the library keeps track itself.
 *  - ready_event (mpsr_squash_decoder_fwd_ex): recorded on `stream` as soon as feat_box3d is complete, so that the
 *    caller can start the FC heads (mpsr_heads_fwd) on ANOTHER stream while the map decoder still runs -- the heads
 *    are many small launches that fill the decoder kernels' partially occupied last rounds (reference graph: the two
 *    branches of net_builder.py:68-89 / monopsr_output_builder.py:126-194 are independent). */
typedef struct mpsr_net_opts {
    float *filter_cache;
    size_t filter_cache_floats;
    int32_t filter_cache_valid;
    mpsr_event_t ready_event;
    /* optional HOST array, one int per layer record (n_layers of the call), zero-initialised by the caller and kept with
     * the cache: the library notes in it WHAT it stored in a layer's slice (F(4x4,3x3) / F(3x3,3x3) transformed filters,
     * the tap GEMM's re-ordered rows) and re-fills a slice whose note does not match what the call is about to read --
     * so a cache survives a change of arithmetic mode, Winograd policy or batch size without the caller tracking it.
     * NULL: filter_cache_valid alone decides. */
    int32_t *filter_cache_tags;
    /* ABI 5: arithmetic mode / Winograd policy of this call (MPSR_CALL_MATH_*, MPSR_CALL_WINOGRAD_*; 0 = the process-wide
     * defaults).  With filter_cache_tags the cache follows a change between calls by itself. */
    int32_t math;
    int32_t winograd_policy;
} mpsr_net_opts;

/* Floats of filter cache that serve every 3x3 layer of `layers` (36 cout cin per dense layer, 25 per atrous one). */
size_t mpsr_filter_cache_floats(const mpsr_layer *layers, int n_layers);

#define MPSR_TRUNK_LAYERS 94 /* root + 30 bottleneck units x 3 + 3 projection shortcuts */

/* Scratch bytes for mpsr_trunk_fwd on a (B,H,W,3) input. */
size_t mpsr_trunk_workspace_bytes(int B, int H, int W);

/* ResNet-101 v1 to block3 at output stride 4 (rates 1/2/4), frozen BatchNorm folded, as
 * FasterRCNNResnet101FeatureExtractor._extract_proposal_features builds it
 * (faster_rcnn_resnet_v1_feature_extractor.py:197-245; resnet_v1.py:79-139,221-236,310-330;
 * resnet_utils.py:176-219).  img (B,H,W,3) -> out (B,H/4,W/4,1024).  layers[] in execution order:
 * root(as 1x1 over im2col, cin=160), then per unit [shortcut?], conv1, conv2, conv3. */
int mpsr_trunk_fwd(const float *img, int B, int H, int W, const float *blob, const mpsr_layer *layers,
                   int n_layers, float *out, void *workspace, size_t workspace_bytes, mpsr_stream_t stream);
/* The same with options (filter cache; ready_event is ignored). */
int mpsr_trunk_fwd_ex(const float *img, int B, int H, int W, const float *blob, const mpsr_layer *layers,
                      int n_layers, float *out, void *workspace, size_t workspace_bytes, const mpsr_net_opts *opts,
                      mpsr_stream_t stream);

#define MPSR_DECODER_LAYERS 7 /* squash 1x1 as two K-halves (crop, full), conv2 x2, conv3 x2, xyz 3x3 */

size_t mpsr_decoder_workspace_bytes(int B, int fh, int fw, int mh, int mw);

/* net_builder.py:62-89 + monopsr_output_builder.py:95-104: concat(crop_feat, full_feat) -> 1x1 conv 512 + ReLU
 * (features_squashed) -> 2x2 max-pool (features_for_box_3d) ; bilinear to (mh/2,mw/2) -> 2x[3x3 conv 256,BN,ReLU]
 * -> bilinear to (mh,mw) -> 2x[3x3 conv 128,BN,ReLU] (features_for_map) -> 3x3 conv 3 (inst_xyz_map_local).
 * crop_feat, full_feat (B,fh,fw,1024).  Outputs: feat_box3d (B,fh/2,fw/2,512), feat_map (B,mh,mw,128) or NULL to
 * skip storing it separately, xyz_map (B,mh,mw,3). */
int mpsr_squash_decoder_fwd(const float *crop_feat, const float *full_feat, int B, int fh, int fw, int mh, int mw,
                            const float *blob, const mpsr_layer *layers, int n_layers, float *feat_box3d,
                            float *feat_map, float *xyz_map, void *workspace, size_t workspace_bytes,
                            mpsr_stream_t stream);
/* Which kernel serves each of the seven layers for this shape (kinds[7], as mpsr_conv2d_plan; 7 = tap GEMM on the
 * source map + gather, csrc/upconv.hip) and the multiply-add FLOPs it issues (executed_flops[7]): throughput accounting
 * for bench.py's roofline object, not needed to run anything. */
int mpsr_squash_decoder_plan(int B, int fh, int fw, int mh, int mw, const mpsr_layer *layers, int n_layers, int *kinds,
                             double *executed_flops);
/* The same with options (filter cache; ready_event = feat_box3d complete). */
int mpsr_squash_decoder_fwd_ex(const float *crop_feat, const float *full_feat, int B, int fh, int fw, int mh, int mw,
                               const float *blob, const mpsr_layer *layers, int n_layers, float *feat_box3d,
                               float *feat_map, float *xyz_map, void *workspace, size_t workspace_bytes,
                               const mpsr_net_opts *opts, mpsr_stream_t stream);

#define MPSR_HEAD_LAYERS 7 /* img_fc (both heads fused along N), prop fc0, fc1, lwh+alpha, reg fc0, fc1, cen_y+cen_z */

typedef struct mpsr_head_consts {
    float image_h, image_w;   /* model_config.image_input_shape (320, 1216) */
    float max_depth;          /* dataset depth_range[1] (45) */
    float cen_y_norm;         /* 1.666754, monopsr_output_builder.py:246 */
    float cen_y_class_offset; /* 0.0648 for Car/kitti, instance_utils.py:933-937 */
    int32_t num_classes;      /* len(dataset_config.classes) */
    int32_t num_alpha_bins;   /* 12 */
} mpsr_head_consts;

size_t mpsr_heads_workspace_bytes(int B, int feat_elems);

/* monopsr_output_builder.py:126-302,407-438,457-488,509-661 wired as monopsr_model.py:320-413 with
 * output_config {lwh: offset, alpha: dc, view_ang: est, cen_x: from_view_ang_and_z, cen_y: offset, cen_z: offset}.
 *   feat_box3d (B,feat_elems) flattened NHWC features_for_box_3d
 *   boxes_2d (B,4) [y1,x1,y2,x2] pixels; cam_p (12) row-major 3x4; view_angs (B); class_idx (B) int32;
 *   mean_lwh (B,3); cen_z_offset (B)
 * Outputs (any may be NULL): lwh (B,3), lwh_offs (B,3), alpha_bins (B,nb), alpha_regs (B,nb), prop_cen_z (B),
 * cen_y (B), cen_y_offs (B), cen_z (B), cen_z_offs (B), cen_x (B), centroids (B,3). */
typedef struct mpsr_head_outputs {
    float *lwh, *lwh_offs, *alpha_bins, *alpha_regs, *prop_cen_z, *cen_y, *cen_y_offs, *cen_z, *cen_z_offs,
        *cen_x, *centroids;
} mpsr_head_outputs;

int mpsr_heads_fwd(const float *feat_box3d, int B, int feat_elems, const float *boxes_2d, const float *cam_p,
                   const float *view_angs, const int *class_idx, const float *mean_lwh, const float *cen_z_offset,
                   const mpsr_head_consts *consts, const float *blob, const mpsr_layer *layers, int n_layers,
                   const mpsr_head_outputs *outs, void *workspace, size_t workspace_bytes, mpsr_stream_t stream);
/* ABI 5: the boxes of several images in one call -- cam_p (n_cams,12), cam_index (B) int32 in [0, n_cams) picks each
 * box's projection matrix (NULL: every box uses the first; an index outside the range is never dereferenced -- the
 * outputs of that box that depend on the projection come back NaN).  The reference feeds one image per step
 * (monopsr_model.py:95-99, one pl_cam_p); N images x 32 boxes in one call read the 150 MB of FC weights once. */
int mpsr_heads_fwd_cams(const float *feat_box3d, int B, int feat_elems, const float *boxes_2d, const float *cam_p,
                        int n_cams, const int *cam_index, const float *view_angs, const int *class_idx,
                        const float *mean_lwh, const float *cen_z_offset, const mpsr_head_consts *consts,
                        const float *blob, const mpsr_layer *layers, int n_layers, const mpsr_head_outputs *outs,
                        void *workspace, size_t workspace_bytes, mpsr_stream_t stream);


/* ---- KITTI object evaluation (scripts/offline_eval/kitti_native_eval/evaluate_object_3d_offline.cpp), fp64 ----
 * One ragged batch of F frames.  Rows hold MPSR_KITTI_FIELDS doubles in the column order below (a detection's score and
 * a ground truth's truncation share a column; a detection's occlusion column is unused); class codes are
 * MPSR_KITTI_CAR ... MPSR_KITTI_OTHER (int32).  Frame f owns detection rows det_off[f] .. det_off[f+1], ground-truth
 * rows gt_off[f] .. gt_off[f+1] and pairs pair_off[f] .. pair_off[f+1]; pair pair_off[f] + j * n_gt(f) + i is
 * (detection j, ground truth i) of the frame.  The offsets come twice: in device memory for the kernels and in host
 * memory, where they are checked (start at 0, never decrease, pair counts = detections x ground truths, end at the row
 * counts) and read before anything is launched.
 * A configuration is (metric, class, difficulty), index (metric * 3 + class) * 3 + difficulty: metric 0 image,
 * 1 bird's-eye view, 2 3D; class 0 car, 1 pedestrian, 2 cyclist; difficulty 0 easy, 1 moderate, 2 hard.
 * min_overlap (host, 9 doubles): MIN_OVERLAP[metric][class] (:55). */
#define MPSR_KITTI_FIELDS 14
#define MPSR_KITTI_X1 0
#define MPSR_KITTI_Y1 1
#define MPSR_KITTI_X2 2
#define MPSR_KITTI_Y2 3
#define MPSR_KITTI_ALPHA 4
#define MPSR_KITTI_H 5
#define MPSR_KITTI_W 6
#define MPSR_KITTI_L 7
#define MPSR_KITTI_TX 8
#define MPSR_KITTI_TY 9
#define MPSR_KITTI_TZ 10
#define MPSR_KITTI_RY 11
#define MPSR_KITTI_SCORE 12
#define MPSR_KITTI_TRUNCATION 12
#define MPSR_KITTI_OCCLUSION 13
enum { MPSR_KITTI_CAR = 0, MPSR_KITTI_PEDESTRIAN = 1, MPSR_KITTI_CYCLIST = 2, MPSR_KITTI_VAN = 3,
       MPSR_KITTI_PERSON_SITTING = 4, MPSR_KITTI_DONTCARE = 5, MPSR_KITTI_OTHER = 6 };
#define MPSR_KITTI_CONFIGS 27
#define MPSR_KITTI_POINTS 41 /* recall sample points; also the most score thresholds of a configuration */
/* the statistics kernels keep one bit per detection of a frame and lane in 64 KB of LDS */
#define MPSR_KITTI_MAX_FRAME_DETECTIONS 8192

typedef struct mpsr_kitti_batch {
    const double *det;            /* (n_det, MPSR_KITTI_FIELDS) */
    const int *det_cls;           /* (n_det) */
    const double *gt;             /* (n_gt, MPSR_KITTI_FIELDS) */
    const int *gt_cls;            /* (n_gt) */
    const int *det_off;           /* (n_frames + 1), device */
    const int *gt_off;            /* (n_frames + 1), device */
    const long long *pair_off;    /* (n_frames + 1), device */
    const int *det_off_host;      /* the same three, host */
    const int *gt_off_host;
    const long long *pair_off_host;
    int n_det, n_gt, n_frames;
} mpsr_kitti_batch;

/* imageBoxOverlap / groundBoxOverlap / box3DOverlap (:228-345) of every pair: overlaps (6, n_pairs) = image, BEV, 3D
 * IoU (criterion -1), then the same over the detection's own area / volume (criterion 0).  BEV: exact clipping of the
 * two rotated rectangles.  A box with non-positive l or w (BEV), or l, w or h (3D), overlaps nothing (0). */
int mpsr_kitti_overlaps(const mpsr_kitti_batch *batch, double *overlaps, mpsr_stream_t stream);

/* computeStatistics with compute_fp = false (:457-636), cleanData (:382-455) applied in the kernel, for every
 * configuration and frame.  tp_scores (27, n_gt): the score of the detection taken as the true positive of each
 * ground-truth row, NaN where there is none; n_care (27, n_frames): the ground truths that count (ignored_gt == 0).
 * A frame with more than MPSR_KITTI_MAX_FRAME_DETECTIONS detections: MPSR_ERR_INVALID_ARG. */
int mpsr_kitti_match(const mpsr_kitti_batch *batch, const double *overlaps, const double *min_overlap,
                     double *tp_scores, int *n_care, mpsr_stream_t stream);

/* Bytes of mpsr_kitti_stats' workspace: the per-frame results of n_configs configurations (those with thresholds). */
size_t mpsr_kitti_stats_workspace_bytes(int n_frames, int n_configs);

/* computeStatistics with compute_fp = true for every configuration, frame and score threshold, summed over frames in
 * frame order (eval_class :686-705).  thresholds (27, MPSR_KITTI_POINTS) device; n_thresholds (27) host, 0..41 (0: the
 * configuration is skipped); compute_aos: the image metric's orientation similarity (0 when a detection has alpha
 * -10).  counts (27, 41, 3) int32 = tp, fp, fn; similarity (27, 41, 2) = orientation similarity (image metric) and
 * heading similarity (BEV, 3D); entries of skipped configurations and thresholds are 0. */
int mpsr_kitti_stats(const mpsr_kitti_batch *batch, const double *overlaps, const double *min_overlap,
                     const double *thresholds, const int *n_thresholds, int compute_aos, int *counts,
                     double *similarity, void *workspace, size_t workspace_bytes, mpsr_stream_t stream);

/* ---- AP by slice (additive to ABI 13): both passes for several slices in one launch each ----
 * A slice is an IoU set and, when depth_tested, a depth bin: a row is in it when lo <= z < hi, z the camera-frame depth
 * (MPSR_KITTI_TZ) of the row itself; the open ends are -inf and +inf, and a NaN z is in no tested bin.  What the C++
 * program prints after two rewrites of the label files defines the result: a ground truth outside the bin gets
 * occlusion 3 (cleanData ignores it: ignored_gt 1 for a row of the evaluated class or its neighbour class, -1 stays -1),
 * a detection outside the bin gets a class nobody evaluates (ignored_det -1, or 1 below the level's minimum height).
 * With depth_tested = 0 no row is tested, a NaN z included: the slice is mpsr_kitti_match / mpsr_kitti_stats with its
 * min_overlap, to the bit.  Those two are this code's one-slice case.
 * A configuration is (slice, one of the 27), index slice * 27 + configuration.  The slice table comes twice, like the
 * batch's offsets: in device memory for the kernels (together with n_thresholds and the list of launched
 * configurations, which the statistics pass writes into its workspace: 32 slices are 864 configurations, more than a
 * launch's arguments should carry) and in host memory, where it is checked before anything is launched:
 * n_slices outside 1 .. MPSR_KITTI_MAX_SLICES, a null table, and a tested slice with hi < lo or a NaN edge are
 * MPSR_ERR_INVALID_ARG with a message. */
#define MPSR_KITTI_MAX_SLICES 32

typedef struct mpsr_kitti_slice {
    double min_overlap[9]; /* MIN_OVERLAP[metric][class] of the slice */
    double lo, hi;         /* the depth bin, lo <= z < hi (read only when depth_tested) */
    int depth_tested;      /* 0: no depth test whatever */
    int reserved;          /* 0 */
} mpsr_kitti_slice;

/* mpsr_kitti_match of every slice: one block per (frame, group of 64 configurations), one lane per configuration.
 * tp_scores (n_slices * 27, n_gt), n_care (n_slices * 27, n_frames): n_care counts the ground truths that are in the
 * slice and pass the level.  tp_scores is written whole, NaN where a row has no true positive (every row of another
 * class): 8 * 27 * n_slices * n_gt bytes, 113 MB at KITTI val's 37 540 ground truths and 14 slices (two IoU sets x
 * ('all' + 6 bins)), and the caller copies as much to the host for getThresholds.  Not shrunk to the rows of the
 * configuration's class: a third of the size, for an index table per class that every caller would have to build. */
int mpsr_kitti_match_slices(const mpsr_kitti_batch *batch, const double *overlaps, const mpsr_kitti_slice *slices,
                            const mpsr_kitti_slice *slices_host, int n_slices, double *tp_scores, int *n_care,
                            mpsr_stream_t stream);

/* Bytes of mpsr_kitti_stats_slices' workspace: the list of launched configurations and the per-frame results of
 * n_configs configurations (those with thresholds, over all slices). */
size_t mpsr_kitti_stats_slices_workspace_bytes(int n_frames, int n_configs);

/* mpsr_kitti_stats of every slice: one block per (frame, launched configuration), one lane per threshold, then the sum
 * over frames in frame order in a second kernel (no float atomics).  thresholds (n_slices * 27, MPSR_KITTI_POINTS) and
 * n_thresholds (n_slices * 27) device; n_thresholds_host the same counts on the host, 0..41 (0: the configuration is
 * skipped -- a class without a detection in the slice).  compute_aos is one flag for the run: a property of all
 * detections, whatever their depth.  counts (n_slices * 27, 41, 3), similarity (n_slices * 27, 41, 2). */
int mpsr_kitti_stats_slices(const mpsr_kitti_batch *batch, const double *overlaps, const mpsr_kitti_slice *slices,
                            const mpsr_kitti_slice *slices_host, int n_slices, const double *thresholds,
                            const int *n_thresholds, const int *n_thresholds_host, int compute_aos, int *counts,
                            double *similarity, void *workspace, size_t workspace_bytes, mpsr_stream_t stream);

/* ---- LiDAR depth maps (ABI 8): demos/depth_completion/save_lidar_depth_maps.py ----
 * Several frames that share one image size (h, w); all maps are (n_frames, h, w) float32. */

/* Bytes of mpsr_lidar_project_depths' workspace: one int per pixel and frame. */
size_t mpsr_lidar_project_workspace_bytes(int n_frames, int h, int w);

/* depth_map_utils.project_depths (monopsr/datasets/kitti/depth_map_utils.py:305-348) of the cloud that
 * get_lidar_point_cloud builds (obj_utils.py:432-450).  points (P, 4) float32 velodyne x y z intensity, frame f owning
 * rows frame_offsets[f] .. frame_offsets[f+1] (device and host copies of the same n_frames + 1 offsets; the host copy is
 * checked: starts at 0, never decreases, at most INT_MAX points per frame).  velo_to_cam0 (n_frames, 3, 4) fp64: rows 0..2
 * of R0_rect . Tr_velo_to_cam composed in 4 x 4 as calib_utils.lidar_to_cam_frame (:311-342) composes it; p2
 * (n_frames, 3, 4) fp64.  In fp64 without contraction: cam0 = T . [x y z 1], pixel = rint(u / w), rint(v / w) of
 * P2 . [cam0 1] (round half to even); a point whose pixel is not finite or lies outside the image is dropped; there is
 * NO z > 0 filter.  Where points share a pixel the LAST one (in cloud order) wins, and the stored value is
 * max_depth - max(0, max_depth - z) rounded once to float32 (a point beyond max_depth stores max_depth); 0 elsewhere. */
int mpsr_lidar_project_depths(const float *points, const long long *frame_offsets, const long long *frame_offsets_host,
                              int n_frames, const double *velo_to_cam0, const double *p2, int h, int w,
                              double max_depth, float *out, void *workspace, size_t workspace_bytes,
                              mpsr_stream_t stream);

#define MPSR_DEPTH_MAX_KERNEL 15
enum { MPSR_DEPTH_BLUR_BILATERAL = 0, MPSR_DEPTH_BLUR_GAUSSIAN = 1 };
enum { MPSR_DEPTH_KERNEL_FAR = 0, MPSR_DEPTH_KERNEL_MED = 1, MPSR_DEPTH_KERNEL_NEAR = 2 };

typedef struct mpsr_depth_fill_opts {
    float max_depth;    /* 100.0 in the reference */
    int extrapolate;    /* 0 / 1 */
    int blur_type;      /* MPSR_DEPTH_BLUR_* */
    int kernel_h[3];    /* dilation kernels far (30 < d), med (15 < d <= 30), near (0.1 < d <= 15): 1 .. 15 */
    int kernel_w[3];
    unsigned char kernels[3][MPSR_DEPTH_MAX_KERNEL * MPSR_DEPTH_MAX_KERNEL]; /* 0/1, row-major, row stride 15 */
} mpsr_depth_fill_opts;

/* Bytes of mpsr_depth_fill_multiscale's workspace (it holds the stage planes when the caller passes no `stages`). */
size_t mpsr_depth_fill_workspace_bytes(int n_frames, int h, int w);

/* IP-Basic's fill_in_multiscale (src/ip_basic/ip_basic.py:40-193) of every frame: depths (n_frames, h, w) -> out.
 * stages, if not null: (n_frames, 8, h, w), the process images s1 .. s8 of show_process.  h, w >= 5; the dilation
 * kernels take cv2's default anchor (kw / 2, kh / 2).  The cv2 calls follow OpenCV's semantics: dilate / erode ignore
 * the image border, medianBlur(5) replicates it, GaussianBlur((5,5), 0) ([1 4 6 4 1] / 16, rows then columns) and
 * bilateralFilter(5, 0.5, 2.0) (13 taps, the 4098-entry colour table of the frame's max - min, sum / wsum in float32)
 * reflect it (BORDER_REFLECT_101).  Every selection stage is exact; DESIGN.md section 7.2 says what the blurs assume. */
int mpsr_depth_fill_multiscale(const float *depths, int n_frames, int h, int w, const mpsr_depth_fill_opts *opts,
                               float *out, float *stages, void *workspace, size_t workspace_bytes,
                               mpsr_stream_t stream);

/* ---- Training ground truth from depth maps (ABI 9): instance images and per-box crops ----
 * Several frames that share one image size (h, w); depth maps (n_frames, h, w) float32 as read_depth_map returns them. */

#define MPSR_INSTANCE_MAX_BOXES 255  /* per frame: value 255 of an instance image is the background */
#define MPSR_INSTANCE_BOX_STRIDE 20  /* doubles per box of mpsr_instance_images' table */
enum { MPSR_CENTROID_BOTTOM = 0, MPSR_CENTROID_MIDDLE = 1 };

/* demos/instances/gen_instance_masks.py:86-153 (depth-map clouds) of every frame -> out (n_frames, h, w) uint8: 255 is
 * background, k the k-th box of the frame.  boxes (n_boxes_total, 20) fp64, frame f owning rows box_offsets[f] ..
 * box_offsets[f+1] (device and host copies; at most 255 per frame): the inflated box's u, up0, up1, v, vp0, vp3, w,
 * wp0, wp4 of obj_utils.points_in_box_3d (:867-910), then the float32 2-D box y1, x1, y2, x2 and one unused double.
 * p2 (n_frames, 3, 4) fp64.  Per pixel (u, v) of depth d: the point of depth_map_utils.get_depth_point_cloud with
 * ratio = d / (float)P[0][0] in float32, x = (u - cu) * ratio + x_offset, y = (v - cv) * ratio in fp64, z = d, rounded
 * to float32 (zero depths included); it belongs to a box when the three slab tests (x a0 + y a1) + z a2 in fp64 hold
 * inclusively and its projection ((p0 x + p1 y) + p2 z) + p3, u' = r0 / r2, v' = r1 / r2 lies in [x1, x2] x [y1, y2].
 * The LAST such box of the frame wins. */
int mpsr_instance_images(const float *depth, int n_frames, int h, int w, const double *p2, const double *boxes,
                         const long long *box_offsets, const long long *box_offsets_host, unsigned char *out,
                         mpsr_stream_t stream);

/* instance_utils.tf_instance_xyz_crop_from_depth_map (instance_utils.py:395-481) of n_boxes boxes across frames, with
 * view_norm=True (xyz_local) and view_norm=False (xyz_global) in one pass.  inst (n_frames, h, w) uint8 instance images;
 * p2 (n_frames, 3, 4) float32; per box: frame_index, instance_id (0..254), boxes_2d [y1, x1, y2, x2] float32, boxes_3d
 * (7) float32, view_angs (the estimated viewing angle).  Device arrays, plus host copies of frame_index, instance_id and
 * boxes_2d for the checks.  The box rounds half to even; rows r0:r2 and columns c0:c2 must be a non-empty part of the
 * image.  The depth masked by inst == id is resized to roi x roi by TF 1.8's resize_nearest_neighbor(align_corners),
 * back-projected at pixel centres of the unrounded box in float32; valid = |d| >= 0.1; both maps are multiplied by valid.
 * The ROI must be square (roi_h == roi_w).  xyz_local / xyz_global (n_boxes, roi, roi, 3), valid (n_boxes, roi, roi, 1);
 * every element is written.  DESIGN.md section 7.3. */
int mpsr_instance_xyz_crops(const float *depth, const unsigned char *inst, const float *p2, int n_frames, int h, int w,
                            const int *frame_index, const int *instance_id, const float *boxes_2d,
                            const float *boxes_3d, const float *view_angs, const int *frame_index_host,
                            const int *instance_id_host, const float *boxes_2d_host, int n_boxes, int roi_h,
                            int roi_w, int centroid_type, int rotate_view, float *xyz_local, float *xyz_global,
                            float *valid, mpsr_stream_t stream);

/* ---- Training samples assembled on the device (ABI 10): oversampling draw, 2-D box jitter, crops without host copies ----
 * Random numbers are counter-based, Philox4x32-10 (multipliers 0xD2511F53, 0xCD9E8D57; key increments 0x9E3779B9,
 * 0xBB67AE85): key = (seed & 0xffffffff, seed >> 32), counter = (draw j, slot s, the frame's index in the split file,
 * (epoch << 4) | stream), stream 0 for the oversampling draw and 1 for the jitter; 0 <= epoch < 2^28.  A uniform is
 * ((w0 >> 5) * 2^26 + (w1 >> 6)) / 2^53 of two words; a pair of normals is Box-Muller in fp64 of (1 - u0, u1), u0 from
 * words 0, 1 and u1 from words 2, 3: r = sqrt(-2 ln(1 - u0)), z0 = r cos(2 pi u1), z1 = r sin(2 pi u1).
 * DESIGN.md section 7.4. */

enum { MPSR_JITTER_NONE = 0, MPSR_JITTER_OVERSAMPLE = 1, MPSR_JITTER_ALL = 2 };

/* The slots of a batch.  Per slot: slot_frame (a row of the per-frame tables, 0 .. n_frames-1) and slot_s (its slot in
 * the frame's sample).  Per-frame tables: num_objs (>= 1), label_offset (the frame's first row of label_boxes),
 * split_index (the RNG coordinate), frame_local (passed through: the frame's index among the frames of its image size),
 * image_hw (n_frames, 2), p00_p02 (n_frames, 2) = P2[0][0], P2[0][2].  label_boxes (n_labels, 4) fp64 x1 y1 x2 y2.
 * kitti_dataset.py:301-308: slot s < num_objs is label s; a later slot is label floor(u * num_objs), u the uniform of
 * draw 0 of stream 0.  jitter_flag: 0 (MPSR_JITTER_NONE), s >= num_objs (MPSR_JITTER_OVERSAMPLE) or 1 (MPSR_JITTER_ALL).
 * Outputs per slot: label_row = label_offset + index, oversample_index, jitter_flag, boxes_xyxy (n, 4) the label's box,
 * slot_hw (n, 2), slot_p (n, 2), slot_split_index, slot_frame_local.
 * THE CALLER MUST GUARANTEE 0 <= slot_frame < n_frames and slot_s >= 0: both arrays are on the device, so this entry
 * point cannot check them and has no status word.  A value out of range is not reported; it is read as frame 0 /
 * slot 0 (so that no lane reads outside the tables) and the slot's outputs are those of that frame, i.e. wrong. */
int mpsr_sample_slots(const int *slot_frame, const int *slot_s, int n, const int *num_objs,
                      const long long *label_offset, const int *split_index, const int *frame_local,
                      const int *image_hw, const double *p00_p02, const double *label_boxes, int n_frames,
                      unsigned long long seed, int epoch, int jitter_mode, long long *label_row, int *oversample_index,
                      int *jitter_flag, double *boxes_xyxy, int *slot_hw, double *slot_p, int *slot_split_index,
                      int *slot_frame_local, mpsr_stream_t stream);

/* kitti_aug.jitter_obj_boxes_2d (kitti_aug.py:173-254) of n slots, one lane per slot, in fp64 and in the reference's
 * order: a slot whose flag is 0 or whose box is under 10 px wide or high keeps its box (0 trials); trial t draws
 * new_centroid_x ~ N(cx, half_w / 3), new_centroid_y ~ N(cy, half_h / 3) (draw 2t of stream 1: z0, z1) and new_half_w ~
 * N(half_w, half_w / 6), new_half_h ~ N(half_h, half_h / 6) (draw 2t + 1), clips to [0, width - 1] x [0, height - 1],
 * and the first trial with evaluation.two_d_iou(new, original) >= iou_threshold_min (in (0, 1]) wins.  The reference
 * loops until then; here a slot that used max_trials trials keeps its box and reports max_trials + 1.
 * Inputs per slot: boxes_xyxy (n, 4) fp64, jitter_flag, image_hw (n, 2), p00_p02 (n, 2), frame_index, slot.
 * Outputs: out_xyxy (n, 4) fp64; out_boxes_2d (n, 4) float32 [y1, x1, y2, x2]; out_boxes_2d_norm = (double)box /
 * (double)dim rounded to float32 (kitti_dataset.py:450); out_view_angs = get_viewing_angle_box_2d of the float32 box;
 * out_trials.  With write_unjittered == 0 the three float32 outputs of a slot that kept its box are left as the caller
 * filled them (the dataset's rows computed on the host). */
int mpsr_jitter_boxes_2d(const double *boxes_xyxy, const int *jitter_flag, const int *image_hw, const double *p00_p02,
                         const int *frame_index, const int *slot, int n, unsigned long long seed, int epoch,
                         double iou_threshold_min, int max_trials, int write_unjittered, double *out_xyxy,
                         float *out_boxes_2d, float *out_boxes_2d_norm, float *out_view_angs, int *out_trials,
                         mpsr_stream_t stream);

/* mpsr_instance_xyz_crops (same kernel, same results) without host copies: the per-box checks are made on the device.
 * A box that fails them is written as zeros and reported in status (2 int32 on the device, which the caller zeroes and
 * reads when it wants to know): status[0] |= MPSR_CROP_BAD_*, status[1] += 1 per such box. */
enum { MPSR_CROP_BAD_FRAME = 1, MPSR_CROP_BAD_ID = 2, MPSR_CROP_BAD_NOT_FINITE = 4, MPSR_CROP_BAD_BOX = 8 };
int mpsr_instance_xyz_crops_status(const float *depth, const unsigned char *inst, const float *p2, int n_frames, int h,
                                   int w, const int *frame_index, const int *instance_id, const float *boxes_2d,
                                   const float *boxes_3d, const float *view_angs, int n_boxes, int roi_h, int roi_w,
                                   int centroid_type, int rotate_view, float *xyz_local, float *xyz_global,
                                   float *valid, int *status, mpsr_stream_t stream);

/* ---- Image noise (ABI 12): kitti_aug.apply_image_noise fused with a batch's frame gather and uint8 -> float32 ----
 * What the reference's function (kitti_aug.py:124-170) does is not what its comments say: each of its five stages
 * computes from the ORIGINAL image and overwrites the result, so only the last stage that fires is seen, and its
 * "swap" of G and B, a tuple assignment on numpy views, copies B into G and leaves B.  The caller chooses:
 *   MPSR_IMAGE_NOISE_REFERENCE  what the function does: the highest-numbered noise stage that fired applied to the
 *                               original pixel; if none fired and the swap did, G := B; otherwise a copy.
 *   MPSR_IMAGE_NOISE_COMPOSED   what it describes: from the original, every fired stage in order acts on the result of
 *                               the one before; the swap exchanges G and B.
 * A noise stage is np.uint8(np.clip(value + noise, 0, 255)): the sum in fp64, the clip, truncation toward zero.
 * Stages (bit of `stages`): 0 swap, p < 0.10; 1 Gaussian per element, sigma 10, p < 0.40; 2 Gaussian per channel,
 * sigma 8, p < 0.40; 3 brightness, one Gaussian, sigma 15, p < 0.40; 4 uniform per element in +-amount,
 * amount = 10 u, p < 0.40.
 * Random numbers as above (key, uniform, normal pair), counter = (c0, c1, the frame's index in the split file,
 * (epoch << 4) | stream) with two more streams:
 *   stream 2, per frame, c1 = 0: c0 = 0 -> random_values[0], [1] (words 0,1 and 2,3); c0 = 1 -> [2], [3];
 *     c0 = 2 -> [4] and amount = 10 * u; c0 = 3 -> a normal pair, the channel offsets R, G (* 8.0);
 *     c0 = 4 -> a normal pair, the channel offset B (* 8.0) and the brightness (* 15.0).
 *   stream 3, per pair of elements, c0 = q for elements 2q, 2q + 1 of the frame flattened H W C, c1 = the stage's bit:
 *     1 -> a normal pair * 10.0; 4 -> -amount + (2 * amount) * u for the call's two uniforms.
 * So an image depends on (seed, epoch, the frame's index in the split file) alone.  Draws of a stage whose result is
 * never seen are not made.
 * frames (n_frames, h, w, 3) uint8; gather (nb) int32 picks the frames, in any order and with repeats; frame_index (nb)
 * int32 is each gathered frame's RNG coordinate.  out (nb, h, w, 3) float32 holds the integers 0 .. 255; stages (nb)
 * int32; params (nb, 5) fp64: amount, the channel offsets R, G, B, the brightness, drawn whether their stage fired or
 * not.  h * w * 3 < 2^31 - 8.
 * THE CALLER MUST GUARANTEE 0 <= gather < n_frames: the array is on the device; a value out of range is read as
 * frame 0.  DESIGN.md section 7.4. */
enum { MPSR_IMAGE_NOISE_REFERENCE = 1, MPSR_IMAGE_NOISE_COMPOSED = 2 };
int mpsr_image_noise(const unsigned char *frames, int n_frames, int h, int w, const int *gather,
                     const int *frame_index, int nb, unsigned long long seed, int epoch, int mode, float *out,
                     int *stages, double *params, mpsr_stream_t stream);

/* ---- Evaluation on 2-D detections (ABI 11): MSCNN merging and the evaluator's detection rows ----
 * DESIGN.md section 7.5. */

enum { MPSR_MERGE_SCORE_DISTANCE = 0, MPSR_MERGE_SCORE_MAX = 1, MPSR_MERGE_SCORE_MIN = 2 };

/* obj_utils.merge_kitti_and_mscnn_obj_labels (obj_utils.py:1037-1089) of n_frames frames in one launch, one wave per
 * frame.  Ragged inputs: frame f owns the labels label_off[f] .. label_off[f+1]-1 of label_boxes (n_labels, 4) float32
 * [y1, x1, y2, x2] and label_z (n_labels) float32 (the labels' t[2]), and the detections det_off[f] .. det_off[f+1]-1
 * of det_boxes (n_dets, 4) float32 [y1, x1, y2, x2] and det_scores (n_dets) fp64, in file order.  Both offset tables
 * hold n_frames + 1 entries on the device.
 * Per detection, in order: two_d_iou (datasets/kitti/evaluation.py:6-44) against the frame's ORIGINAL label boxes --
 * products, union and quotient in float32, the quotient widened to fp64 and rounded to 3 decimals, rint(x * 1000) /
 * 1000 --, the arg-max with the lowest index on ties, and, when iou >= min_iou, the label's box, score and match index
 * are overwritten.  Then every label whose score is exactly 0 gets, in float32,
 * min(max(1 - z / 45, 0.1), 1) (MPSR_MERGE_SCORE_DISTANCE), 1 (_MAX), or stays 0 (_MIN).
 * Outputs per label: out_boxes (n_labels, 4) float32, out_scores (n_labels) fp64, out_match (n_labels) int32: the
 * detection's index within its frame, or -1.  A frame without labels merges nothing (the reference's np.argmax raises).
 * THE CALLER MUST GUARANTEE that both offset tables are non-decreasing and end at n_labels / n_dets; a frame whose
 * offsets leave the tables is not reported: its labels are left unwritten (label offsets) or it is merged with no
 * detection (detection offsets). */
int mpsr_merge_detections(const float *label_boxes, const float *label_z, const long long *label_off,
                          long long n_labels, const float *det_boxes, const double *det_scores,
                          const long long *det_off, long long n_dets, int n_frames, double min_iou, int score_type,
                          float *out_boxes, double *out_scores, int *out_match, mpsr_stream_t stream);

/* evaluator_utils.kitti_label_array of n prediction rows in one launch, one lane per row.  box_3d (n, 9) float32
 * [x y z l w h ry score class] and box_2d (n, 7) float32 [y1 x1 y2 x2 alpha score class] as mpsr_format_boxes leaves
 * them.  Every value is widened to fp64 and rounded as np.round(v, 3) rounds it: rint(v * 1000) / 1000.
 * rows (n, MPSR_KITTI_FIELDS) fp64 in the evaluator's column order (x1 y1 x2 y2 alpha h w l x y z ry score 0);
 * cls (n) = (int)class; keep (n) = score >= score_threshold, in fp64 on the unrounded score.
 * project != 0: the 2-D box is evaluator_utils.project_boxes_3d of the 3-D box with the frame's p2 (n_frames, 12) fp64
 * and image_wh (n_frames, 2) int32 [width, height], frame (n) picking the frame: the clipped extent of the eight
 * projected corners, and keep also needs the box at least partly inside the image and, before clipping, no wider or
 * taller than 0.8 of it.  A row whose frame is outside [0, n_frames) is not kept.  frame, p2 and image_wh may be null
 * when project == 0. */
int mpsr_kitti_detection_rows(const float *box_3d, const float *box_2d, const int *frame, const double *p2,
                              const int *image_wh, int n, int n_frames, double score_threshold, int project,
                              double *rows, int *cls, int *keep, mpsr_stream_t stream);

/* ---- The evaluator's per-object error statistics (additive to ABI 13) ----
 * The reference's save_metrics (core/evaluator_utils.py:294-403) over a device-resident table: values (n_rows, n_cols)
 * float32, row-major, one row per object; frame (n_rows) int32 in [0, n_frames), the rows of a frame in any order and
 * not necessarily adjacent.  column_metric (n_cols) is a HOST array: column c feeds metric column_metric[c] in
 * [0, n_metrics); several columns may feed one metric (its values are then the columns flattened), a metric without a
 * column has count 0.  n_cols <= MPSR_METRIC_STATS_MAX_COLS.
 * nan_rule MPSR_NAN_RULE_ENTRY leaves out the NaN entries alone; frame, n_frames and frame_flags are not used and may
 * be null / 0.  MPSR_NAN_RULE_FRAME is the reference's rule (core/evaluator.py:270-281): one NaN among a frame's values
 * of a metric, over all the metric's columns, leaves out all of that frame's values of that metric; a row whose frame
 * is outside [0, n_frames) is left out as well.  frame_flags: caller-owned scratch of n_metrics * n_frames int32,
 * overwritten.
 * stats (n_metrics, 6) fp64: count, mean, std (population, np.std), mean of |x|, std of |x|, dropped = the number of
 * values left out.  count 0 gives NaN in the four statistics.  Every element is written on every call (n_rows == 0
 * included).  fp64 throughout, two passes (the mean, then the centred squares), one workgroup per metric, a fixed
 * summation order and no atomics: two calls on one table return the same bits.  DESIGN.md section 7.5. */
enum { MPSR_NAN_RULE_ENTRY = 0, MPSR_NAN_RULE_FRAME = 1 };
#define MPSR_METRIC_STATS_MAX_COLS 32
int mpsr_metric_stats(const float *values, const int *frame, int n_rows, int n_cols, const int *column_metric,
                      int n_metrics, int n_frames, int nan_rule, int *frame_flags, double *stats,
                      mpsr_stream_t stream);

/* ---- Each predicted box against its own label (additive to ABI 13) ----
 * n objects, one lane each, every value widened from float32 to fp64 first.  pred_box_3d and gt_box_3d (n, 7)
 * [x y z l w h ry], y on the bottom face: the first seven columns of mpsr_format_boxes' box_3d and the label's
 * boxes_3d row.  fed_box_2d (n, 4) [y1 x1 y2 x2], the box the network was fed, or null.  label_info (n, 6)
 * [truncation, occlusion, x1, y1, x2, y2] of the KITTI label itself, or null.  depth_edges and box_iou_edges are HOST
 * arrays of at most MPSR_OBJECT_PAIRS_MAX_EDGES finite, strictly increasing doubles (a count of 0: one bin).
 * overlaps (n, 4) fp64: iou_2d_fed = mpsr_kitti_overlaps' image IoU of the fed box against the label's own box (NaN
 * when either pointer is null or one of the eight values is not finite); iou_bev and iou_3d = that entry point's BEV
 * and 3-D IoU (criterion -1, the same arithmetic: exact polygon clipping, non-positive l / w, or l / w / h, give 0);
 * centre_dist = sqrt((dx dx + dy dy) + dz dz) between the box centres, y at half height.  A field among the two 3-D
 * boxes that is not finite makes the last three NaN.
 * table (n, 9) float32: those four rounded, then hit3d_70, hit3d_50, hit3d_25, hitbev_70, hitbev_50: 1.0 or 0.0 from
 * `>=` on the fp64 IoU, NaN where the IoU is NaN.
 * bins (n, 3) int32: depth = the number of depth_edges <= the label's z (a z on an edge goes to the upper bin; -1
 * when z is not finite); difficulty = the KITTI program's level of the label's own box, height y2 - y1 in fp64:
 * 0 height > 40, occlusion <= 0, truncation <= 0.15; 1 height > 25, <= 1, <= 0.3; 2 height > 25, <= 2, <= 0.5;
 * otherwise 3 (-1 when label_info is null or one of the row's six values is not finite); the truncation limits are
 * taken rounded to float32, as the truncation itself arrives, so that a label on a limit stays on it; fed_box = the number of
 * box_iou_edges <= iou_2d_fed (-1 when that is NaN).
 * Every output element is written on every call; n == 0 is a no-op.  Argument errors (negative n, a null box or
 * output pointer with n > 0, edges that are too many, not finite or not increasing) are reported before any launch.
 * DESIGN.md section 7.11. */
#define MPSR_OBJECT_PAIRS_MAX_EDGES 15
int mpsr_object_pairs(const float *pred_box_3d, const float *gt_box_3d, const float *fed_box_2d,
                      const float *label_info, int n, const double *depth_edges, int n_depth_edges,
                      const double *box_iou_edges, int n_box_iou_edges, double *overlaps, float *table, int *bins,
                      mpsr_stream_t stream);

/* mpsr_metric_stats under MPSR_NAN_RULE_ENTRY for several sets of rows ("slots") in one launch.  values, n_rows,
 * n_cols, column_metric (HOST) and n_metrics as there.  bins (n_rows, n_axes) int32: the row's bin on every axis;
 * axis_bins (n_axes) is a HOST array, the number of bins of each axis.  n_axes <= MPSR_METRIC_STATS_MAX_AXES, the sum
 * of axis_bins <= MPSR_METRIC_STATS_MAX_BINS: more is an argument error, nothing is truncated.
 * stats (1 + sum of axis_bins, n_metrics, 6) fp64, the six statistics of mpsr_metric_stats per (slot, metric): slot 0
 * is every row, then axis 0's bins, axis 1's bins, ...  A row whose index on an axis is negative or >= axis_bins[a] is
 * in none of that axis' bins (and still in slot 0); a row outside a slot is neither counted nor dropped there.  A
 * slot without a value has count 0 and NaN in the four statistics.  Every element is written on every call.
 * One workgroup per (slot, metric), each with mpsr_metric_stats' element-to-thread assignment and summation tree, no
 * atomics: slot 0 holds the bits mpsr_metric_stats returns for the same table under MPSR_NAN_RULE_ENTRY, and two calls
 * return the same bits.  bins may be null when no axis has a bin.  DESIGN.md section 7.11. */
#define MPSR_METRIC_STATS_MAX_AXES 4
#define MPSR_METRIC_STATS_MAX_BINS 64
int mpsr_metric_stats_binned(const float *values, const int *bins, int n_rows, int n_cols, const int *column_metric,
                             int n_metrics, int n_axes, const int *axis_bins, double *stats, mpsr_stream_t stream);

/* ---- One step's row of the training log (additive to ABI 13) ----
 * Writes row `row` of the caller-owned table rows (n_rows, n_cols) float32, row-major, n_cols == n_terms +
 * MPSR_TRAIN_LOG_STAT_COLS, and steps[row] = step (steps: n_rows int64); no other element of either is touched.  One
 * launch of one workgroup, no host synchronisation, no allocation: a training loop logs its losses without waiting for
 * them (core/train_log.py).
 * Columns [0, n_terms): the DEVICE scalars *terms.p[i] (the step's loss terms and their total); a null pointer writes
 * NaN, "term absent this step".  The struct is passed BY VALUE; entries from n_terms on are not read.
 * The other five columns come from sumsq, the first n_segments floats of the clip table's scratch, where
 * mpsr_clip_adam_ema_step / mpsr_clip_by_norm_segments leave the squared norm of every variable's reduced, unclipped
 * gradient:
 *   n_terms + 0  grad_norm         sqrt(sum_s (double)sumsq[s]), rounded to float32
 *   n_terms + 1  max_var_norm      the largest sqrtf(sumsq[s])
 *   n_terms + 2  n_clipped         the number of s with sqrtf(sumsq[s]) > clip_norm (strict, as the clip itself compares);
 *                                  0 when clip_norm <= 0
 *   n_terms + 3  n_nonfinite_vars  the number of s whose sumsq[s] is NaN or +-inf; these are left out of the three above
 *   n_terms + 4  lr
 * sumsq == NULL or n_segments == 0: 0 in the four gradient columns.  The sum is fp64 in a fixed order (strided per-thread
 * partials, then a tree over LDS), no atomics: two calls on the same inputs return the same bits.
 * MPSR_ERR_INVALID_ARG before any launch: n_terms outside [1, MPSR_TRAIN_LOG_MAX_TERMS], n_cols != n_terms +
 * MPSR_TRAIN_LOG_STAT_COLS, row outside [0, n_rows), null rows / steps, n_segments < 0. */
#define MPSR_TRAIN_LOG_MAX_TERMS 16
#define MPSR_TRAIN_LOG_STAT_COLS 5
typedef struct { const float *p[MPSR_TRAIN_LOG_MAX_TERMS]; } mpsr_train_log_terms;
int mpsr_train_log_append(mpsr_train_log_terms terms, int n_terms, const float *sumsq, int n_segments, float clip_norm,
                          float lr, long long step, float *rows, long long *steps, int n_rows, int n_cols, int row,
                          mpsr_stream_t stream);

/* ---- Scene reconstruction (additive to ABI 13): instance clouds, z-buffer depth maps and instance images ----
 * A chunk of n_frames frames, frame f of frame_hw[f] = (h, w) pixels, its pixels at pixel_offset[f] ..
 * pixel_offset[f + 1] of every per-pixel array (pixel_offset[0] = 0, pixel_offset[n_frames] = total_pixels); n_boxes
 * boxes of points_per_box points each, box b of frame box_frame[b], box_frame never decreasing.  Arrays named *_host
 * are host copies of the device array of the same name, checked before anything is launched.  The three calls share
 * one caller-owned workspace and run in this order on one stream: project, then resolve and / or compact.
 * Empty sizes (n_frames, n_boxes or points_per_box 0) are no-ops that return MPSR_OK; negative sizes, null pointers
 * with non-empty sizes, n_boxes * points_per_box >= 2^32 and a frame of more than 2^30 pixels are
 * MPSR_ERR_INVALID_ARG.  DESIGN.md section 7.7. */

/* Bytes of the workspace: one uint64 key per pixel, one int32 pixel index per point, n_frames + 1 first-box indices
 * and n_boxes + 1 int64 box offsets.  0 for empty or refused sizes. */
size_t mpsr_scene_workspace_bytes(int n_frames, long long total_pixels, int n_boxes, int points_per_box);

/* xyz_global (n_boxes, points_per_box, 3) float32 in the camera frame; valid_mask (n_boxes, points_per_box) float32 or
 * null (all valid); box_keep (n_boxes) int32 or null (all kept); cam_p (n_frames, 3, 4) fp64.  Per point, in fp64
 * without contraction: u_k = ((P[k][0] x + P[k][1] y) + P[k][2] z) + P[k][3], col = rint(u0 / u2), row = rint(u1 / u2)
 * (half to even).  A point is KEPT when its box is kept, its mask is > 0, x, y and z are finite, z > 0, u2 > 0,
 * 0 <= col < w and 0 <= row < h.  A kept point stores its pixel index row * w + col in the workspace (a dropped one -1)
 * and lowers its pixel's key, ((uint64) float_bits(z) << 32) | (b * points_per_box + p), with an unsigned 64-bit
 * atomicMin: the nearer point wins, on equal float32 depth the lower point index.  (mpsr_lidar_project_depths keeps the
 * LAST duplicate of a pixel instead.) */
int mpsr_scene_project(const float *xyz_global, const float *valid_mask, const int *box_frame,
                       const int *box_frame_host, const int *box_keep, const double *cam_p, const int *frame_hw,
                       const int *frame_hw_host, const long long *pixel_offset, const long long *pixel_offset_host,
                       int n_frames, int n_boxes, int points_per_box, void *workspace, size_t workspace_bytes,
                       mpsr_stream_t stream);

/* depth (total_pixels) float32: the winner's z bit for bit, 0 for a pixel no kept point fell on; instance
 * (total_pixels) uint8: the winner box's ordinal within its frame, 255 for such a pixel (the ground-truth instance
 * images' convention).  A frame of more than MPSR_INSTANCE_MAX_BOXES boxes is MPSR_ERR_INVALID_ARG. */
int mpsr_scene_resolve(const int *box_frame, const int *box_frame_host, int n_frames, long long total_pixels,
                       int n_boxes, int points_per_box, const void *workspace, size_t workspace_bytes, float *depth,
                       unsigned char *instance, mpsr_stream_t stream);

/* The kept points (visible_only: the pixels' winners only) in box order and, within a box, point order.  kept_per_box
 * and visible_per_box (n_boxes) int32 are both written whatever visible_only says.  Of the M selected points: xyz
 * (M, 3) float32 the input values copied; rgb (M, 3) float32 = images[f][3 * pixel + c], images a device table of
 * n_frames pointers to (h, w, 3) float32 images (nearest pixel; images and rgb both null: no colours); box (M) int32;
 * pixel (M) int32 = row * w + col; frame_offset (n_frames + 1) int64: frame f owns rows frame_offset[f] ..
 * frame_offset[f + 1], frame_offset[n_frames] = M.  The output buffers hold n_boxes * points_per_box rows; rows from M
 * on are not written.  Counts, a one-workgroup scan and ranks from wave ballots: no atomics, and two calls return the
 * same bytes. */
int mpsr_scene_compact(const float *xyz_global, const int *box_frame, const float *const *images,
                       const long long *pixel_offset, int n_frames, long long total_pixels, int n_boxes,
                       int points_per_box, int visible_only, void *workspace, size_t workspace_bytes, float *xyz,
                       float *rgb, int *box, int *pixel, long long *frame_offset, int *kept_per_box,
                       int *visible_per_box, mpsr_stream_t stream);

/* ---- Scoring a reconstruction against ground truth (additive to ABI 13) ----
 * Runs after mpsr_scene_project on the same stream and workspace (which holds the keys and the per-point pixel
 * indices), independent of resolve and compact, in any order.  gt_depth / gt_instance: device tables of n_frames
 * pointers to the frames' (h, w) float32 LiDAR depth maps and uint8 instance images (no alignment is asked of the
 * images: the histogram pass peels to 16 bytes).  box_gt_id (n_boxes) int32: the value box b has in its frame's
 * instance image; anything outside [0, 254] means "no ground truth for this box".  xyz_global is the array project
 * took; it is checked and not read (a winner's z is its key's upper half).
 * With f = box_frame[b], g = box_gt_id[b], a KEPT point and its pixel `at` as project stored them, a VISIBLE point its
 * pixel's winner ((key & 0xffffffff) == b * points_per_box + p), counts (n_boxes, 6) int32, all exact:
 *   0 kept       kept points (= kept_per_box of compact)
 *   1 on_points  kept points with gt_instance[f][at] == g (0 when g is "none")
 *   2 pred_px    visible points: the pixels the box wins (= visible_per_box)
 *   3 inter_px   visible points with gt_instance[f][at] == g
 *   4 gt_px      pixels of frame f whose instance value is g (0 when g is "none")
 *   5 depth_n    the points of inter_px whose d = gt_depth[f][at] is finite and > 0
 * sums (n_boxes, 3) fp64 over the depth_n points, e = (double)z - (double)d with z the point's float32 z: the sums of
 * e, |e| and e * e (the square rounded before it is added).
 * scratch: mpsr_scene_score_scratch_bytes(n_frames) bytes, the (n_frames, 256) int32 value counts of the instance
 * images; the call zeroes it and fills it with integer atomics (LDS and global), whose result does not depend on
 * order.  The per-box part is one launch of one workgroup per box: counts from wave ballots, the fp64 sums per thread
 * in slice order, then a lane-ordered wave reduction, wave partials through LDS and a combine in wave order.  No
 * floating-point atomics: two calls on the same inputs return the same bytes.
 * Checked on the host before any launch: empty sizes (and total_pixels 0) are no-ops that return MPSR_OK and write
 * nothing; negative sizes, null pointers with non-empty sizes, n_boxes * points_per_box >= 2^32 and a box_frame_host
 * out of [0, n_frames) or decreasing are MPSR_ERR_INVALID_ARG; a workspace smaller than mpsr_scene_workspace_bytes or
 * a scratch smaller than mpsr_scene_score_scratch_bytes is MPSR_ERR_WORKSPACE. */
size_t mpsr_scene_score_scratch_bytes(int n_frames); /* 256 int32 per frame; 0 for n_frames <= 0 */
int mpsr_scene_score(const float *xyz_global, const int *box_frame, const int *box_frame_host, const int *box_gt_id,
                     const float *const *gt_depth, const unsigned char *const *gt_instance,
                     const long long *pixel_offset, int n_frames, long long total_pixels, int n_boxes,
                     int points_per_box, const void *workspace, size_t workspace_bytes, void *scratch,
                     size_t scratch_bytes, int *counts, double *sums, mpsr_stream_t stream);

/* ---- Instance maps rendered as surfaces (additive to ABI 13) ----
 * The same chunk as above, but a box's points are a (map_h, map_w) grid (points_per_box = map_h * map_w, row-major)
 * whose cells are joined into triangles and rasterised through a 64-bit z-buffer of their own.  Cell (i, j),
 * 0 <= i < map_h - 1, 0 <= j < map_w - 1, has the corners v00 = (i, j), v01 = (i, j + 1), v10 = (i + 1, j),
 * v11 = (i + 1, j + 1) and gives triangle k = 0: (v00, v01, v10) and k = 1: (v11, v10, v01); the triangle id is
 * t = ((b (map_h - 1) + i) (map_w - 1) + j) 2 + k.  The workspace is separate from mpsr_scene_workspace_bytes': both
 * renderings of a chunk can coexist.  render, then resolve and / or score, on one stream.
 * Checked on the host before any launch, by every entry point: map_h or map_w < 2 and
 * n_boxes (map_h - 1) (map_w - 1) 2 >= 2^32 are MPSR_ERR_INVALID_ARG, like negative sizes, null pointers with
 * non-empty sizes and a box_frame_host out of range or decreasing; n_frames or n_boxes 0 is a no-op; a workspace
 * smaller than mpsr_scene_surface_workspace_bytes is MPSR_ERR_WORKSPACE. */

/* Bytes of the workspace: one uint64 key per pixel, one (int32, int32) vertex per map point, n_frames + 1 first-box
 * indices, and per box a triangle count and a pixel rectangle.  0 for empty or refused sizes. */
size_t mpsr_scene_surface_workspace_bytes(int n_frames, long long total_pixels, int n_boxes, int map_h, int map_w);

/* The arguments of mpsr_scene_project, and max_edge_dz (float32, > 0, +inf allowed; NaN or <= 0 is
 * MPSR_ERR_INVALID_ARG) and max_span_px (1..1024, else MPSR_ERR_INVALID_ARG).
 * Vertices: u as in mpsr_scene_project.  A vertex is VALID when its box is kept, its mask is > 0, x, y and z are
 * finite, z > 0, u2 > 0, |u0 / u2| < 2^20 and |u1 / u2| < 2^20 (it need not be inside the image).  A valid vertex has
 * the fixed-point screen coordinates X = (int) rint((u0 / u2) 256.0), Y = (int) rint((u1 / u2) 256.0) (half to even):
 * the centre of pixel (col, row) is (256 col, 256 row).
 * A triangle (a, b, c) is DROPPED when a vertex is invalid; when max(z) - min(z) of its three float32 depths, taken in
 * float32, is > max_edge_dz; when its doubled area A = (bX - aX)(cY - aY) - (bY - aY)(cX - aX) (int64) is 0; or when
 * its pixel extent in columns or rows, floor(max / 256) - ceil(min / 256) + 1 (unclamped), exceeds max_span_px.  Every
 * other triangle is DRAWN (an extent <= 0 covers no pixel centre and draws nothing).  With A < 0, b and c are swapped.
 * Coverage of the pixel centre s, over the extent clamped to the image: E(p, q, s) = (qX - pX)(sY - pY) -
 * (qY - pY)(sX - pX), e0 = E(b, c, s), e1 = E(c, a, s), e2 = E(a, b, s), all exact; covered when every e_k > 0, or
 * e_k == 0 and the edge p -> q owns its boundary: qY - pY > 0, or qY - pY == 0 and qX - pX < 0.
 * Depth, fp64 without contraction: q = (e0 (1.0 / za) + e1 (1.0 / zb)) + e2 (1.0 / zc), zf = (float)(A / q).  The key
 * ((uint64) float_bits(zf) << 32) | t is lowered with an unsigned 64-bit atomicMin: the nearer surface wins, on equal
 * float32 depth the lower triangle id.  Per box, by integer atomics: the number of drawn triangles and the rectangle
 * (min / max column and row) of their clamped extents.  Two calls return the same bytes. */
int mpsr_scene_surface_render(const float *xyz_global, const float *valid_mask, const int *box_frame,
                              const int *box_frame_host, const int *box_keep, const double *cam_p, const int *frame_hw,
                              const int *frame_hw_host, const long long *pixel_offset,
                              const long long *pixel_offset_host, int n_frames, int n_boxes, int map_h, int map_w,
                              float max_edge_dz, int max_span_px, void *workspace, size_t workspace_bytes,
                              mpsr_stream_t stream);

/* depth (total_pixels) float32: the key's upper half, 0 for an empty pixel; instance (total_pixels) uint8: the winner
 * box's ordinal within its frame, 255 for an empty pixel; tri (total_pixels) int32 or null: the winner's t, -1 for an
 * empty pixel.  A frame of more than MPSR_INSTANCE_MAX_BOXES boxes is MPSR_ERR_INVALID_ARG. */
int mpsr_scene_surface_resolve(const int *box_frame, const int *box_frame_host, int n_frames, long long total_pixels,
                               int n_boxes, int map_h, int map_w, const void *workspace, size_t workspace_bytes,
                               float *depth, unsigned char *instance, int *tri, mpsr_stream_t stream);

/* The surfaces against ground truth: gt_depth, gt_instance, box_gt_id and scratch (mpsr_scene_score_scratch_bytes) as
 * mpsr_scene_score takes them.  counts (n_boxes, 5) int32, exact: 0 tris (drawn triangles), 1 pred_px (pixels the box
 * wins), 2 inter_px (won pixels whose instance value is g), 3 gt_px (pixels of the frame whose value is g; 0 when g is
 * outside [0, 254]), 4 depth_n (inter_px pixels whose ground-truth depth d is finite and > 0).  sums (n_boxes, 3)
 * fp64 over the depth_n pixels, e = (double)zf - (double)d: the sums of e, |e| and e * e (the square rounded first).
 * One workgroup per box walks the box's rectangle row-major in slices of 256 pixels; each thread adds in slice order,
 * then a lane-ordered wave reduction and a combine in wave order: no floating-point atomics, two calls return the
 * same bytes.  A scratch that is too small is MPSR_ERR_WORKSPACE.  box_gt_id, gt_depth and gt_instance all null: no
 * ground truth (tris and pred_px alone, the other counts and the sums 0, no scratch needed); one or two of them null
 * is MPSR_ERR_INVALID_ARG. */
int mpsr_scene_surface_score(const int *box_frame, const int *box_frame_host, const int *box_gt_id,
                             const float *const *gt_depth, const unsigned char *const *gt_instance,
                             const int *frame_hw, const long long *pixel_offset, int n_frames, long long total_pixels,
                             int n_boxes, int map_h, int map_w, const void *workspace, size_t workspace_bytes,
                             void *scratch, size_t scratch_bytes, int *counts, double *sums, mpsr_stream_t stream);

/* ---- The surfaces as meshes (additive to ABI 13) ----
 * Runs after mpsr_scene_surface_render on the same stream, the same inputs and the same max_edge_dz and max_span_px,
 * and reads that call's workspace (the vertex table and the keys); its own workspace is separate.
 * A triangle t is IN THE MESH when it is DRAWN under mpsr_scene_surface_render's rule (one device function decides
 * both) and, with visible_only != 0, the low 32 bits of at least one key of its frame equal t: it won a pixel.  A map
 * point is a VERTEX when at least one of the (up to six) triangles it is a corner of is in the mesh; no other point
 * appears in the output.
 * Vertices are written frame after frame, box after box, in map-point order; faces frame after frame, box after box,
 * in triangle-id order.  Of the V vertices: xyz (V, 3) float32, the input bits; rgb (V, 3) float32 =
 * images[f][3 (row w + col) + c] at row = rint(u1 / u2), col = rint(u0 / u2) (u as in mpsr_scene_project, half to
 * even), (0, 0, 0) where that pixel is outside the frame or images is null; normal (V, 3) float32; vertex_box (V)
 * int32 = b.  Of the F faces: faces (F, 3) int32 = the corners (a, c, b) of mpsr_scene_surface_render's (a, b, c) --
 * k = 0: (v00, v10, v01), k = 1: (v11, v01, v10); with x right, y down and z forward (c - a) x (b - a) of an unfolded
 * grid points toward the camera -- as FRAME-LOCAL indices, the vertex's rank among its frame's vertices; face_box (F)
 * int32 = b.  The order is never swapped by the sign of the screen area: a fold shows as a flipped normal.
 * normal: the sum, in increasing triangle id, of (c - a) x (b - a) over the vertex's triangles in the mesh, in fp64
 * from the float32 coordinates without contraction (differences, products, then u_y v_z - u_z v_y and so on), divided
 * by its fp64 length sqrt((n_x n_x + n_y n_y) + n_z n_z), each component rounded once; (0, 0, 0) when the length is 0
 * or not finite.  area_per_box (n_boxes) fp64 = the sum of 0.5 |(c - a) x (b - a)| over the box's faces: thread
 * n % 256 adds the box's triangle n in increasing n, then mpsr_scene_surface_score's lane-ordered wave reduction and
 * combine in wave order.
 * vertex_box_offset / face_box_offset (n_boxes + 1) and vertex_frame_offset / face_frame_offset (n_frames + 1) int64:
 * box b owns rows box_offset[b] .. box_offset[b + 1], frame f rows frame_offset[f] .. frame_offset[f + 1]; the last
 * entries are V and F.  As with mpsr_scene_compact the vertex outputs hold n_boxes map_h map_w rows and the face
 * outputs n_boxes 2 (map_h - 1)(map_w - 1) rows; rows from V and F on are not written, and the caller reads the
 * totals from the offset tables.  One byte flag per triangle set by plain stores, counts and ranks from wave ballots,
 * one-workgroup scans: no atomics, and two calls return the same bytes.
 * Checked on the host before any launch: what mpsr_scene_surface_render checks (map_h or map_w < 2, the 2^32 triangle
 * ids, max_edge_dz NaN or <= 0, max_span_px outside 1..1024, null pointers, the frame tables);
 * n_boxes map_h map_w > INT_MAX is MPSR_ERR_INVALID_ARG; either workspace too small is MPSR_ERR_WORKSPACE.  n_boxes or
 * n_frames 0 returns MPSR_OK with the offset tables zeroed (a null table is left alone) and nothing else written. */

/* Bytes of the mesh workspace: one byte per triangle, one int32 rank per map point, two int32 counts per box.  0 for
 * empty or refused sizes. */
size_t mpsr_scene_surface_mesh_workspace_bytes(int n_boxes, int map_h, int map_w);

int mpsr_scene_surface_mesh(const float *xyz_global, const int *box_frame, const int *box_frame_host,
                            const double *cam_p, const int *frame_hw, const int *frame_hw_host,
                            const long long *pixel_offset, const long long *pixel_offset_host,
                            const float *const *images, int n_frames, int n_boxes, int map_h, int map_w,
                            float max_edge_dz, int max_span_px, int visible_only, const void *render_workspace,
                            size_t render_workspace_bytes, void *mesh_workspace, size_t mesh_workspace_bytes,
                            float *xyz, float *rgb, float *normal, int *vertex_box, int *faces, int *face_box,
                            double *area_per_box, long long *vertex_box_offset, long long *vertex_frame_offset,
                            long long *face_box_offset, long long *face_frame_offset, mpsr_stream_t stream);

/* ---- Fitting a centroid to its 2-D box (additive to ABI 13) ----
 * The reference's inference-time projection alignment (core/instances/instance_metrics.py np_proj_error and
 * scipy_proj_error*, datasets/kitti/instance_utils.py proj_points and get_exp_proj_uv_map).  Per box: local (h w, 3)
 * float32 points in map order (point i at row i / w, column i % w), x = [xz_dist d, centroid_y cy, viewing_angle va],
 * a 2-D box [y1, x1, y2, x2], cameras as mpsr_proj_err_norm_cams takes them (an index outside [0, n_cams) is never
 * dereferenced), mask (b, h w) float32 or NULL.
 * The objective, float32 products each rounded: r = R_y(va) p (r = p with rotate_view 0); g = r + (d sin va, cy,
 * d cos va); valid = |r_x| + |r_y| + |r_z| > 0.1 and mask != 0; with cam0_shift g_x += -P[0,3] / P[0,0];
 * (U, V, Wc) = P (g, 1); u = U / Wc, v = V / Wc; the expected grid is np.linspace's start + index * step over the box
 * (rounded half to even with round_box_2d): from the first to the last pixel's top-left corner, or centre with
 * use_pixel_centres.  err = sum over valid points of |u - eu| + |v - ev|, divided by their number; the sum is fp64 in
 * a fixed order without atomics.  No valid point: err = NaN.  A valid point with Wc <= 0: err = +inf. */

/* uv (b, 2, h w) float32 or NULL (0 at points that are not valid), valid (b, h w) uint8 or NULL, err (b) fp64.  A box
 * whose camera index is out of range gets NaN uv, valid 0 and err NaN. */
int mpsr_proj_points(const float *local, const float *x, const float *boxes_2d, const float *cam_p, int n_cams,
                     const int *cam_index, const float *mask, float *uv, unsigned char *valid, double *err, int b,
                     int h, int w, int rotate_view, int cam0_shift, int round_box_2d, int use_pixel_centres,
                     mpsr_stream_t stream);

/* Nelder-Mead on that objective over (d, cy) (n_fit 2) or (d, cy, va) (n_fit 3), one workgroup per box, h w <= 2304.
 * SciPy's rule: vertices x0 and x0 with coordinate k times 1.05 (0.00025 where it is 0); reflection 1, expansion 2,
 * contractions 0.5, shrink 0.5; vertices stably ordered by value; stop when max |x_i - x_best| <= xatol and
 * max |f_i - f_best| <= fatol, or at max_iter iterations or evaluations (<= 0: 200 n_fit; an evaluation past the cap
 * ends the iteration where it stands).  The simplex is fp64; the objective is taken at its float32 rounding; an
 * evaluation without a valid point ranks as +inf.
 * x (b, 3) float32 (va copied through with n_fit 2), err and err0 (b) fp64: the objective at x and at x0, the bits
 * mpsr_proj_points returns there, err <= err0; iters, evals (b) int32 (SciPy's nit and nfev); status (b) int32: 0
 * converged, 1 stopped at the cap, 2 no valid point at x0 or camera index out of range (x = x0, err = err0 = NaN,
 * iters 0, evals 1 or, for the camera, 0). */
int mpsr_proj_fit(const float *local, const float *x0, const float *boxes_2d, const float *cam_p, int n_cams,
                  const int *cam_index, const float *mask, int b, int h, int w, int n_fit, int rotate_view,
                  int cam0_shift, int round_box_2d, int use_pixel_centres, double xatol, double fatol, int max_iter,
                  float *x, double *err, double *err0, int *iters, int *evals, int *status, mpsr_stream_t stream);

/* ---- Shape scores over valid points (additive to ABI 13) ----
 * n boxes, each with a cloud a (n, P, 3) and a cloud b (n, Q, 3), float32; mask_a (n, P) and mask_b (n, Q) float32 or
 * null.  By convention a is the prediction and b the ground truth.
 * Valid point: its mask entry is > 0 (a null mask is all ones, a NaN entry is not valid) and its three coordinates
 * are finite.
 * Nearest distance: for a valid a_i, d_a[i] = the minimum over the valid b_j of the float32 squared distance in
 * mpsr_nn_distance_fwd's arithmetic: float differences, float products, (dx dx + dy dy) + dz dz, nothing contracted;
 * d_b[j] the same in the other direction.  An overflow to +inf propagates.  With null masks and finite clouds d_a
 * and d_b are mpsr_nn_distance_fwd's dist1 and dist2, bit for bit.
 * thresholds: a HOST array of T <= MPSR_SHAPE_MAX_THRESHOLDS finite distances > 0, strictly increasing.
 * counts (n, 2 + 2T) int32: n_a, n_b (the valid points), then within_a[t] = the number of valid a_i with
 * (double) d_a[i] <= thresholds[t] * thresholds[t] (an fp64 product and an fp64 compare), then within_b[t].
 * sums (n, 6) fp64: sum of sqrt((double) d_a), sum of (double) d_a, the same two for b, max d_a, max d_b.
 * table (n, 5 + 3T) float32, computed in fp64 from counts and sums and rounded once: accuracy = sum sqrt d_a / n_a,
 * completeness = sum sqrt d_b / n_b, chamfer_l1 = (accuracy + completeness) / 2, chamfer_sq = sum d_a / n_a +
 * sum d_b / n_b, hausdorff = sqrt(max(max d_a, max d_b)), then per threshold precision = within_a / n_a, recall =
 * within_b / n_b, fscore = 2 p r / (p + r) (0 when p + r == 0).
 * dist_a (n, P) and dist_b (n, Q) float32, or null: every point's d, NaN at the points that are not valid.
 * Empty side (n_a == 0 or n_b == 0, P == 0 or Q == 0 included): the box's six sums and its table row are NaN, its
 * within counts 0, its dist rows NaN; n_a and n_b are still reported.
 * Every output element is written on every call; n == 0 is a no-op that returns MPSR_OK.  workspace: 8-byte aligned,
 * mpsr_shape_scores_workspace_bytes(n, P, Q, T) bytes (0 for n == 0 and for refused sizes), overwritten.
 * MPSR_ERR_INVALID_ARG before any launch: negative sizes, a null cloud or output pointer with a non-empty size, T
 * outside [0, MPSR_SHAPE_MAX_THRESHOLDS], thresholds that are not finite, not > 0 or not strictly increasing,
 * n max(P, Q) >= 2^31.  MPSR_ERR_WORKSPACE: a workspace that is too small.
 * One workgroup per (box, direction, slab of 1024 queries) leaves integer counts and fp64 partial sums in the
 * workspace; a second kernel adds them in slab order.  fp64 sums in a fixed order, no floating-point atomics: two
 * calls on the same inputs return the same bytes.  Cost to know: a box with an empty side is still searched, and with
 * dist_a / dist_b given its rows are then rewritten with NaN by one thread, P + Q single stores. */
#define MPSR_SHAPE_MAX_THRESHOLDS 8
size_t mpsr_shape_scores_workspace_bytes(int n, int P, int Q, int T);
int mpsr_shape_scores(const float *a, const float *mask_a, int P, const float *b, const float *mask_b, int Q, int n,
                      const double *thresholds, int T, void *workspace, size_t workspace_bytes, int *counts,
                      double *sums, float *table, float *dist_a, float *dist_b, mpsr_stream_t stream);

/* ---- Shape scores against surfaces (additive to ABI 13) ----
 * mpsr_shape_scores' statistics, the distance of a valid point taken to the other side's SURFACE: its valid points
 * and its kept triangles.  n boxes, each with two grids a and b (n, h, w, 3) float32, h, w >= 1, row-major (point i at
 * row i / w, column i % w); mask_a and mask_b (n, h w) float32 or null.  By convention a is the prediction and b the
 * ground truth.  Valid point: mpsr_shape_scores' rule (mask entry > 0, a null mask is all ones, a NaN entry is not
 * valid, and the three coordinates are finite).
 * Triangles of a grid: mpsr_scene_surface_render's indexing.  Cell (i, j), 0 <= i < h - 1, 0 <= j < w - 1, has the
 * corners v00 = (i, j), v01 = (i, j + 1), v10 = (i + 1, j), v11 = (i + 1, j + 1) and gives k = 0: (v00, v01, v10) and
 * k = 1: (v11, v10, v01), with the id t = ((i (w - 1)) + j) 2 + k within the box.  A triangle (A, B, C) is KEPT if and
 * only if its three vertices are valid and each of its edges (A, B), (B, C), (C, A) has (double) len2 <= max_edge *
 * max_edge, len2 the float32 squared length in mpsr_nn_distance_fwd's arithmetic, float differences, float products,
 * (dx dx + dy dy) + dz dz (an overflow to +inf is kept by max_edge = +inf alone); the product max_edge * max_edge and
 * the compare are fp64.  max_edge: a host double >= 0, +inf allowed.  The rule is a 3-D edge length, the same in every
 * frame; it is not mpsr_scene_surface_render's max_edge_dz / max_span_px, which are properties of one view.
 * Distance of a valid query q of one side against the other side:
 *   d = min((double) d_point, min over the kept triangles (A, B, C) of their edge and face terms),
 * d_point exactly mpsr_shape_scores' float32 nearest-valid-point distance (+inf where the other side has no valid
 * point); the terms in fp64 on the coordinates converted exactly, every dot product x.y = (x0 y0 + x1 y1) + x2 y2,
 * every product and sum rounded once, nothing contracted:
 *   edge (U, V) for (A, B), (B, C), (C, A): e = V - U, w = q - U, ee = e.e, t = w.e; if ee > 0 && t > 0 && t < ee:
 *     s = t / ee, r = w - s e (r_k = w_k - s e_k), the term is r.r; otherwise no term.
 *   face: e0 = B - A, e1 = C - A, n = e0 x e1 = (e0_1 e1_2 - e0_2 e1_1, e0_2 e1_0 - e0_0 e1_2, e0_0 e1_1 - e0_1 e1_0),
 *     nn = n.n, d00 = e0.e0, d01 = e0.e1, d11 = e1.e1, den = d00 d11 - d01 d01, w = q - A, d20 = w.e0, d21 = w.e1,
 *     v = d11 d20 - d01 d21, u = d00 d21 - d01 d20; if nn > 0 && den > 0 && v > 0 && u > 0 && v + u < den:
 *     hq = w.n, the term is (hq hq) / nn; otherwise no term.
 * A minimum does not depend on its order and no term is NaN or -0 (float32 coordinates cannot overflow these fp64
 * expressions), so d is defined bit for bit.  Consequences: a valid point that no kept triangle uses stays part of the
 * surface, as a point; d <= (double) d_point always; at max_edge = 0 every d equals (double) d_point bit for bit (a
 * kept triangle then has three equal corners, ee = nn = 0, and adds nothing -- short of distinct corners less than
 * 2^-74 apart, whose float32 squares underflow to 0 while their fp64 ones do not); a degenerate triangle (ee = 0 on an
 * edge, nn = 0 or den <= 0) adds no term of that kind and divides nothing by zero.
 * thresholds: as mpsr_shape_scores takes them.  counts (n, 2 + 2T) int32: n_a, n_b, within_a[t] = the number of valid
 * a_i with d_a[i] <= thresholds[t] * thresholds[t] (fp64), within_b[t].  sums (n, 6) fp64: sum of sqrt(d_a), sum of
 * d_a, the same two for b, max d_a, max d_b (fp64).  table (n, 5 + 3T) float32: mpsr_shape_scores' formulas on these
 * counts and sums, hausdorff = sqrt(max(max d_a, max d_b)).  dist_a, dist_b (n, h w) FP64, or null: every point's d,
 * NaN at the points that are not valid.  tri_counts (n, 2) int32: the kept triangles of a and of b.
 * Empty side (n_a == 0 or n_b == 0): the six sums and the table row NaN, the within counts 0, the dist rows NaN; n_a,
 * n_b and tri_counts are still reported.  A side with valid points and no kept triangle is not empty: it is a cloud.
 * Every output element is written on every call; n == 0 is a no-op that returns MPSR_OK.  workspace: 8-byte aligned,
 * mpsr_surface_scores_workspace_bytes(n, h, w, T) bytes (0 for n <= 0 and for refused sizes), overwritten.
 * MPSR_ERR_INVALID_ARG before any launch: n < 0, h or w < 1, a null grid or output pointer with n > 0, T outside
 * [0, MPSR_SHAPE_MAX_THRESHOLDS], thresholds mpsr_shape_scores would refuse, max_edge NaN or < 0, h w > 2^30 or
 * n h w >= 2^31.  MPSR_ERR_WORKSPACE: a workspace that is too small.
 * One workgroup per (box, direction, slab of 512 queries) takes the point minimum, then works out and compacts the
 * searched grid's kept triangle records 256 ids at a time in LDS (ranks from ballots) and runs its queries over them;
 * a second kernel adds the slabs' partials in slab order.  No floating-point atomics: two calls on the same inputs
 * return the same bytes.  Cost to know: every (query, kept triangle) pair is evaluated, nothing is pruned. */
size_t mpsr_surface_scores_workspace_bytes(int n, int h, int w, int T);
int mpsr_surface_scores(const float *a, const float *mask_a, const float *b, const float *mask_b, int n, int h, int w,
                        const double *thresholds, int T, double max_edge, void *workspace, size_t workspace_bytes,
                        int *counts, double *sums, float *table, double *dist_a, double *dist_b, int *tri_counts,
                        mpsr_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MONOPSR_HIP_H */
