/*
 * azula_amd -- C ABI of the MI355X (gfx950) sampling hot path.
 *
 * The reference (probabilists/azula, /root/reference) is pure Python and has NO FFI: its
 * "operator boundary" is the duck-typed protocol Schedule / Denoiser / Sampler
 * (azula/noise.py:49-63, azula/denoise.py:97-114, azula/sample.py:54-161).  This header is
 * the boundary a maintainer would bind (ctypes stub in INTEGRATION.md) to replace the ATen
 * op sequences that protocol dispatches per sampling step.  Each entry point cites the
 * reference lines whose arithmetic it replaces.
 *
 * Contract of every function below:
 *   - plain C, raw DEVICE pointers + sizes + POD structs + a hipStream_t (passed as void*);
 *   - returns 0 on success, a negative AZ_E_* argument error, or a positive hipError_t;
 *   - never allocates, never synchronises, never throws, keeps no mutable global state,
 *     is re-entrant and hipGraph-capturable (workspace is supplied by the caller);
 *   - tensors are fp32 unless the entry point's name says otherwise (`_f64`: fp64 latents of a Sampler(dtype=float64);
 *     `_bf16_f32` / `_f16_f32`: half-precision MFMA operands packed by az_pack_conv_weight_half_f32, fp32 activations and
 *     accumulation).  "NHWC" tensors have a channel stride that is a multiple of 4 floats (zero-filled pad channels), so
 *     every access is a 16-byte vector.
 */
#ifndef AZULA_AMD_H
#define AZULA_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AZ_VERSION 1

enum {
  AZ_OK = 0,
  AZ_E_NULL = -1,      /* required pointer is NULL            */
  AZ_E_SHAPE = -2,     /* inconsistent / unsupported shape    */
  AZ_E_ALIGN = -3,     /* pointer or stride not 16-B aligned  */
  AZ_E_UNSUPPORTED = -4
};

typedef void* az_stream_t; /* hipStream_t */

int az_version(void);
const char* az_error_string(int code);

/* ------------------------------------------------------------------ per-step scalars
 * One row per sampling step, computed on the HOST with torch-CPU 0-d ops in the
 * reference's op order (azula/noise.py:125-129, azula/denoise.py:309-312,
 * azula/plugins/adm/__init__.py:109-114, azula/sample.py:249-253) and uploaded once --
 * the analogue of the reference's single `time_pairs` H2D copy (azula/sample.py:151).   */
typedef struct AzStepCoef {
  float c_in;      /* backbone input scale for THIS step                                  */
  float c_skip;    /* mean = c_skip * x_t + c_out * F                                      */
  float c_out;
  float c_time;    /* Karras: log(sigma_t / alpha_t)                                       */
  float alpha_t;
  float alpha_s;
  float k_x;       /* sigma_s * sqrt(1 - tau) / sigma_t                                    */
  float k_eps;     /* sigma_s * sqrt(tau)                                                  */
  float c_in_next; /* c_in of the NEXT step (pre-scaled second output), 0 on the last step */
  float clip_lo;   /* mean clip (ADM eval, plugins/adm/__init__.py:133-134); -inf/+inf = off */
  float clip_hi;
  float guidance;  /* CFG strength (azula/guidance/cfg.py:63-65)                           */
  int32_t time_index; /* ADM: searchsorted(sigmas, sigma_t * c_in)                          */
  int32_t step;       /* step number (informational)                                        */
  float pad[2];
} AzStepCoef; /* 64 bytes */

/* cur[0] = table[*step_counter]; *step_counter += 1.  One thread; first node of a step
 * graph, so that the same captured graph can be replayed for every step.               */
int az_step_begin(AzStepCoef* cur, const AzStepCoef* table, int32_t* step_counter, int32_t n_steps,
                  az_stream_t stream);

/* ------------------------------------------------------------------ K1: fused transition
 * Replaces, in ONE pass over the latent (12 B/element for DDIM eta=0, 16 B with eps):
 *   azula/denoise.py:322            mean = c_skip*x_t + c_out*F   [ADM: clip, plugins/adm/__init__.py:126-134]
 *   azula/guidance/cfg.py:63-65     mean = mean_p + g*(mean_p - mean_n)        (if F_neg != NULL)
 *   azula/sample.py:257-259         x_s = alpha_s*mean + k_x*(x_t - alpha_t*mean) + k_eps*eps
 *   azula/denoise.py:317 (next step) xin = c_in_next * x_s                      (if xin_next != NULL)
 * Arithmetic is done with separately rounded mul/add in the reference's association order,
 * so the result is bit-identical to the torch-CPU op sequence for the same inputs.
 *
 * Flat form: x_t, F, F_neg, eps, x_s, xin_next all have n elements.
 * F may have `f_channels` >= channels per sample (ADM learn_var: 6 of which 3 are used):
 *   F element (b, c, i) is at F[(b*f_channels + c)*inner + i], x at (b*channels + c)*inner + i. */
typedef struct AzTransitionArgs {
  const float* x_t;
  const float* F;      /* backbone output (positive branch)            */
  const float* F_neg;  /* backbone output (negative CFG branch) or NULL */
  const float* eps;    /* noise or NULL (treated as 0: DDIM eta = 0)    */
  float* x_s;          /* may alias x_t                                 */
  float* xin_next;     /* optional: c_in_next * x_s, same layout as x_s unless nhwc_pad > 0 */
  float* mean_out;     /* optional: posterior mean (for Denoiser.forward), same layout as x_s */
  int64_t batch, channels, inner; /* x is (batch, channels, inner)      */
  int64_t f_channels;  /* channels of F per sample (>= channels)        */
  int32_t f_nhwc;      /* 1: F is NHWC with channel stride f_channels (backbone-native layout) */
  int32_t nhwc_pad;    /* >0: xin_next is written NHWC with this channel stride (zero pad)    */
  const AzStepCoef* coef; /* DEVICE pointer                              */
} AzTransitionArgs;
int az_transition_f32(const AzTransitionArgs* args, az_stream_t stream);

/* ---- linear multistep update ------------------------------------------------
 * Replaces the per-step tensor arithmetic of the Adams-Bashforth sampler family:
 *   zABSampler.__call__   azula/sample.py:519-546     vABSampler.__call__   azula/sample.py:593-620
 *   zEABSampler.__call__  azula/sample.py:688-715     xEABSampler.__call__  azula/sample.py:797-821
 *   REABSampler.__call__  azula/sample.py:915-950
 * which all have the form (prediction linear in x_t and the posterior mean, history of <= order
 * predictions, x_s linear in x_t and the history):
 *   pred = a x_t + b mean                      -> written to `pred` (its history slot)
 *   x_s  = p x_t + sum_j w_j hist[j] + w_new pred
 * `coef` is a DEVICE pointer to 4 + n_hist floats [a, b, p, w_new, w_0 .. w_{n_hist-1}] (the
 * fp64 Vandermonde solves of `_adams_bashforth` stay on the host, azula/sample.py:486-508).
 * x_s may alias x_t; pred must not alias any hist[j].  All pointers 16-byte aligned.          */
#define AZ_MULTISTEP_MAX_HIST 7
typedef struct AzMultistepArgs {
  float* x_s;
  float* pred;
  const float* x_t;
  const float* mean;
  const float* hist[AZ_MULTISTEP_MAX_HIST]; /* older predictions, oldest first */
  const float* coef;                        /* DEVICE pointer                  */
  int64_t count;                            /* elements                        */
  int32_t n_hist;                           /* 0 .. AZ_MULTISTEP_MAX_HIST      */
  int32_t pad_;
} AzMultistepArgs;
int az_multistep_f32(const AzMultistepArgs* args, az_stream_t stream);

/* ---- RePaint masked resample --------------------------------------------------------------------
 * Replaces the per-iteration tensor arithmetic of RePaintSampler.step (azula/guidance/repaint.py:51-61), one pass over n
 * elements behind each DDIM step:
 *   x_s' = mask ? alpha_s * y + sigma_s * n_y : x_s                    -> x_s_out   (repaint.py:53-57, torch.where)
 *   x_t' = (alpha_t / alpha_s) * x_s' + (alpha_t * sqrt(...)) * n_x    -> x_t_out   (repaint.py:59-61)
 * Separately rounded mul / add in the reference's association order and a select (not a blend), so the result is
 * bit-identical to the torch op sequence on the same inputs.  `coef` is a DEVICE pointer to the four host-computed 0-d values
 * [alpha_s, sigma_s, alpha_t / alpha_s, alpha_t * sqrt((sigma_t / alpha_t)^2 - (sigma_s / alpha_s)^2)].  `mask` holds one
 * byte per element (a contiguous bool tensor, 4-byte aligned); every float pointer is 16-byte aligned.  Either output may be
 * NULL (not both) and either may alias x_s; n_x is read only when x_t_out != NULL (the last iteration keeps x_s' only). */
typedef struct AzRepaintArgs {
  const float* x_s;    /* the DDIM step's x_s                          */
  const float* y;      /* observation, n elements                      */
  const uint8_t* mask; /* 1 byte per element, nonzero = observed        */
  const float* n_y;    /* randn_like(y)                                */
  const float* n_x;    /* randn_like(x_s), or NULL without x_t_out      */
  float* x_s_out;      /* optional: x_s'                               */
  float* x_t_out;      /* optional: x_t'                               */
  const float* coef;   /* DEVICE pointer, 4 floats                     */
  int64_t n;
} AzRepaintArgs; /* 72 bytes */
int az_repaint_f32(const AzRepaintArgs* args, az_stream_t stream);

/* ---- Measurement operators of the guidance methods (csrc/operators.hip, azula_amd/guidance/operators.py) -----------
 * The linear maps A of inpainting, super-resolution and deblurring with their adjoints, on planar fp32 (B, C, H, W) tensors
 * seen as planes = B * C contiguous images of H x W.  The project's own: the reference takes A as a Python callable.  No
 * atomics and a fixed summation order (two launches give the same bits); any plane count (work items are a linear 64-bit
 * range); tensors 16-byte aligned, tap vectors 4-byte aligned (else AZ_E_ALIGN).
 *
 * az_op_mul_f32: y[i] = x[i] * m[i mod m_n] -- a mask whose shape is a suffix of x's; m_n divides n (else AZ_E_SHAPE).  m is
 * read 16 bytes at a time where m_n % 4 == 0.  y may be x.
 *
 * az_op_avgpool_f32: y[n, i, j] = (sum_{a < fh} sum_{b < fw} x[n, i fh + a, j fw + b]) * (1 / (fh fw)), summed in that order in
 * fp32; y is (planes, H / fh, W / fw).  1 <= fh, fw <= 16, H % fh == 0 and W % fw == 0 (else AZ_E_SHAPE).
 *
 * az_op_avgpool_adj_f32: dx[n, Y, X] = scale * g[n, Y / fh, X / fw] on the (H, W) grid, g being (planes, H / fh, W / fw):
 * scale = 1 / (fh fw) is the adjoint of az_op_avgpool_f32, scale = 1 its pseudo-inverse (nearest up-sampling).
 *
 * az_op_blur_f32: the separable correlation y[n, i, j] = sum_a taps_h[a] sum_b taps_w[b] x~[n, i + a - nh / 2, j + b - nw / 2] of
 * x's size, x~ = 0 outside the image (circular = 0) or wrapped (circular = 1: nh / 2 < H and nw / 2 < W).  nh, nw odd, 1 .. 65
 * (else AZ_E_SHAPE); taps are DEVICE pointers, arbitrary values.  y must not overlap x (AZ_E_SHAPE).  One launch: a workgroup
 * stages its tile and halo in LDS, runs the row pass into LDS and the column pass to y; both sums are chains of fused
 * multiply-adds from 0 with the taps ascending.  The adjoint is the same entry with both tap vectors reversed.
 *
 * az_op_blur_tile: the output tile (rows th, columns tw) of a launch with these tap counts (host arithmetic).
 *
 * az_op_psf_f32: the general (non-separable) correlation y[b, c, i, j] = sum_a sum_b' k[a, b'] x~[b, c, i + a - kh / 2,
 * j + b' - kw / 2] on (B, C, H, W), k = psf + (b psf_bstride + c psf_cstride) kh kw: the strides count PSFs and 0 shares the PSF
 * along that axis (one PSF for all planes, one per channel, one per sample, one per plane).  x~ as for az_op_blur_f32; kh, kw
 * odd, 1 .. 65, strides >= 0 (else AZ_E_SHAPE); psf is a DEVICE pointer, 4-byte aligned, arbitrary values; y must not overlap x
 * (AZ_E_SHAPE).  Replaces F.conv2d(groups = planes) on a padded copy (motion deblurring: one 61 x 61 kernel per image).  Each
 * output is ONE chain of kh kw fused multiply-adds from 0, a ascending and then b' ascending.  A workgroup stages its tile and
 * halo in LDS; a thread carries up to 4 output rows of a column, so one staged value feeds up to 4 chains.  The adjoint is the
 * same entry on the PSF flipped along both axes, for both paddings.
 *
 * az_op_psf_tile: the output tile (rows th, columns tw) of an az_op_psf_f32 launch with this PSF size (host arithmetic).
 *
 * az_op_decimate_f32: y[n, i, j] = x[n, i fh + oh, j fw + ow], y being (planes, H / fh, W / fw) -- the slice x[..., oh::fh,
 * ow::fw].  1 <= fh, fw <= 16, 0 <= oh < fh, 0 <= ow < fw, H % fh == 0 and W % fw == 0 (else AZ_E_SHAPE); y must not overlap x.
 * A copy: no arithmetic.
 *
 * az_op_decimate_adj_f32: dx = g zero-stuffed back onto the (H, W) grid: dx[n, i fh + oh, j fw + ow] = g[n, i, j] and 0
 * elsewhere; EVERY element of dx is written.  The adjoint of az_op_decimate_f32 and, as A A^T = I, its pseudo-inverse; replaces
 * zeros() and a strided assignment.  The same constraints.
 *
 * az_op_chanmix_f32: y[b, o, p] = sum_c M[o Cin + c] x[b, c, p] on x (B, Cin, HW), y (B, Cout, HW) -- a per-pixel channel mix
 * (colourisation: 3 -> 1), what einsum("oc,bcp->bop") computes.  M is a DEVICE pointer, 4-byte aligned; 1 <= Cin, Cout <= 16
 * (else AZ_E_SHAPE); y must not overlap x.  Each output is a chain of fused multiply-adds from 0 with c ascending; 16 bytes
 * along p at a time where HW % 4 == 0, one pixel per thread otherwise.  The adjoint is the same entry with M^T (Cin and Cout
 * exchanged), the pseudo-inverse the same entry with M^+. */
int az_op_mul_f32(float* y, const float* x, const float* m, int64_t n, int64_t m_n, az_stream_t stream);
int az_op_avgpool_f32(float* y, const float* x, int64_t planes, int64_t H, int64_t W, int32_t fh, int32_t fw,
                      az_stream_t stream);
int az_op_avgpool_adj_f32(float* dx, const float* g, int64_t planes, int64_t H, int64_t W, int32_t fh, int32_t fw, float scale,
                          az_stream_t stream);
int az_op_blur_f32(float* y, const float* x, const float* taps_h, int32_t nh, const float* taps_w, int32_t nw, int64_t planes,
                   int64_t H, int64_t W, int32_t circular, az_stream_t stream);
int az_op_blur_tile(int32_t nh, int32_t nw, int32_t* th, int32_t* tw);
int az_op_psf_f32(float* y, const float* x, const float* psf, int32_t kh, int32_t kw, int64_t psf_bstride, int64_t psf_cstride,
                  int64_t B, int64_t C, int64_t H, int64_t W, int32_t circular, az_stream_t stream);
int az_op_psf_tile(int32_t kh, int32_t kw, int32_t* th, int32_t* tw);
int az_op_decimate_f32(float* y, const float* x, int64_t planes, int64_t H, int64_t W, int32_t fh, int32_t fw, int32_t oh,
                       int32_t ow, az_stream_t stream);
int az_op_decimate_adj_f32(float* dx, const float* g, int64_t planes, int64_t H, int64_t W, int32_t fh, int32_t fw, int32_t oh,
                           int32_t ow, az_stream_t stream);
int az_op_chanmix_f32(float* y, const float* x, const float* M, int64_t B, int32_t Cin, int32_t Cout, int64_t HW,
                      az_stream_t stream);

/* ---- Batched 2-D DFT of the Fourier-domain operators (csrc/fft.hip; FourierOperator, MRIOperator) -------------------
 * az_op_fft2_f32: dst[k, l] = scale * sum_{m, n} src[m, n] exp(-+ 2 pi i (k m / H + l n / W)) on every plane, "-" for inverse = 0
 * and "+" for inverse = 1, the DC term at [0, 0].  SPLIT-complex fp32: the real and the imaginary parts are separate planes, and
 * plane (b, c), b < B, c < C, of a tensor starts at base + b * bstride + c * H * W floats, so the two halves of a (B, 2 C, H, W)
 * tensor are a destination or a source (bstride = 2 C H W).  src_im == NULL: real input (4 bytes read per element); dst_im ==
 * NULL: only the real part is written.  H and W are powers of two in 1 .. AZ_OP_FFT2_MAX, inverse is 0 or 1, B, C > 0, and for
 * B > 1 the strides are at least C H W (else AZ_E_SHAPE); dst_re and src_re are required, and `work` where az_op_fft2_work says
 * so and dst_im is NULL (else AZ_E_NULL); every base is 16-byte aligned (else AZ_E_ALIGN); no destination, source or `work` plane
 * may share a float with another (AZ_E_SHAPE): never in place.  Planes of at most 8192 points run whole in LDS in one launch
 * (12 bytes per element real -> complex); larger ones in two, rows and then tiles of 8192 / H columns, with the row result in
 * dst_re and in dst_im (or `work`): 28 bytes per element.  Stockham radix-4 stages (one radix-2 stage for an odd log2), twiddles
 * from sincospif of the exact fraction: multiples of a quarter turn are exactly 0 / +-1, so H, W <= 4 are exact on integers.  No
 * atomics, a fixed order of operations: a plane's result does not depend on the other planes of the launch.
 *
 * az_op_fft2_work: the floats of `work` such a call may need (0: none; else B C H W, dense).  Host arithmetic. */
#define AZ_OP_FFT2_MAX 1024
int az_op_fft2_f32(float* dst_re, float* dst_im, int64_t dst_bstride, const float* src_re, const float* src_im,
                   int64_t src_bstride, float* work, int64_t B, int64_t C, int32_t H, int32_t W, int32_t inverse, float scale,
                   az_stream_t stream);
int az_op_fft2_work(int64_t B, int64_t C, int32_t H, int32_t W, int64_t* floats);

/* ---- Coil maps of multi-coil (SENSE) MRI (csrc/coil.hip; MultiCoilMRIOperator) -----------------------------------------
 * y_k = M F (S_k . x), k < K, with complex sensitivity maps S_k.  SPLIT-complex fp32 in az_op_fft2_f32's plane convention: plane
 * (b, k) of a tensor starts at base + b * bstride + k * HW floats and the real and imaginary parts have separate bases, so the two
 * halves of a (B, 2 K, H, W) tensor are a destination or a source.  HW is any plane size (not only a power of two).
 *
 * az_op_coil_expand_f32: dst[b, k] = S[b, k] . x[b].  Replaces the torch sequence torch.complex(x_re, x_im)[:, None] * maps
 * followed by the split into .real / .imag that torch.fft-based SENSE code writes (four elementwise launches and a (B, K, H, W)
 * complex temporary).  x_im == NULL: a real image.  With x = a + i b and S = c + i d: re = fma(a, c, -(b d)), im = fma(a, d, b c);
 * real image: re = a c, im = a d (single roundings).  (4 or 8) + 16 K bytes per pixel.
 *
 * az_op_coil_combine_f32: dst[b] = sum_k conj(S[b, k]) . z[b, k], the transpose of expand as a real-linear map.  Replaces
 * (maps.conj() * z).sum(1) and, with normalize = 1, the division by (maps.abs() ** 2).sum(1) of the coil-combined zero-filled
 * reconstruction.  dst_im == NULL: the real part only.  With z = p + i q, from 0 with k ascending: re = fma(c, p, re), re =
 * fma(d, q, re); im = fma(c, q, im), im = fma(-d, p, im).  normalize = 1 accumulates D = sum_k (c^2 + d^2) with fmas in the same
 * loop and writes acc / D (IEEE division), or 0 where D == 0.  16 K + (4 or 8) bytes per pixel.  No atomics: a fixed order.
 *
 * s_bstride = 0: one set of maps for the whole batch; >= K HW: per-sample maps.  Bases and strides that are multiples of 4 floats
 * with HW % 4 == 0 take 16-byte loads and stores, anything else a scalar form.  K >= 1, B, HW >= 0 (an empty tensor launches
 * nothing and returns AZ_OK), strides >= 0 and, for B > 1, at least the tensor's K HW or HW floats, normalize 0 or 1 (else
 * AZ_E_SHAPE); every pointer but x_im (expand) and dst_im (combine) is required -- the product with a complex map is complex, and
 * coil data is complex (AZ_E_NULL); pointers are 4-byte aligned (AZ_E_ALIGN); no destination plane shares a float with the other
 * destination or with a source (AZ_E_SHAPE). */
int az_op_coil_expand_f32(float* dst_re, float* dst_im, int64_t dst_bstride, const float* x_re, const float* x_im,
                          int64_t x_bstride, const float* s_re, const float* s_im, int64_t s_bstride, int64_t B, int32_t K,
                          int64_t HW, az_stream_t stream);
int az_op_coil_combine_f32(float* dst_re, float* dst_im, int64_t dst_bstride, const float* z_re, const float* z_im,
                           int64_t z_bstride, const float* s_re, const float* s_im, int64_t s_bstride, int64_t B, int32_t K,
                           int64_t HW, int32_t normalize, az_stream_t stream);

/* ---- Parallel-beam Radon transform of the computed-tomography operator (csrc/radon.hip; RadonOperator) ---------------
 * Planes of H x W fp32 (`planes` contiguous images) and sinograms of A x D fp32 (A angles, D detector bins, `planes` contiguous
 * sinograms).  The model is pixel driven with linear interpolation on the detector and its weights are fp32 by definition: with
 * (c, s) = table[2 a], table[2 a + 1], x = j - (W - 1) / 2, y = i - (H - 1) / 2,
 *   p = fadd(fmul(fadd(fmul(x, c), fmul(y, s)), inv_spacing), (D - 1) / 2),   w(a, k, i, j) = max(0, fsub(1, |fsub(p, float(k))|)),
 * every operation rounded on its own.  Both maps evaluate w with one device function, so the back-projector's matrix is exactly
 * the transpose of the projector's; sums are chains of fused multiply-adds from 0 in a fixed order, no atomics, and a plane's
 * result does not depend on the other planes of the launch.
 * PRECONDITION: every table row is (cos, sin) of an angle, rounded to fp32 -- max(|c|, |s|) >= sqrt(1/2) is what bounds the
 * projector's window; rows that are not are memory safe (every read is bounds checked) but lose weights.
 *
 * az_op_radon_f32: dst[n, a, k] = sum_{i, j} w(a, k, i, j) src[n, i, j].  One output per thread; the sum walks the major axis
 * (rows where |c| >= |s|, else columns) ascending and, on each line, floor(2 h) + 3 candidates ascending from floor(n0 - h), n0
 * the solution of p = k on that line and h = 1 / (inv_spacing max(|c|, |s|)).  Column-major angles read a transposed copy of the
 * planes that the call makes in `work` (required: az_op_radon_work floats), so that their reads coalesce as the row-major ones do.
 *
 * az_op_radon_adj_f32: dst[n, i, j] = scale * sum_{a, k} w(a, k, i, j) src[n, a, k].  One pixel per thread; angles ascending,
 * bins floor(p) and floor(p) + 1 (all that can have a weight), guarded by 0 <= k < D.
 *
 * az_op_radon_filter_f32: dst[r, s] = scale * sum_k taps[|s - k|] src[r, k] on `rows` rows of D, k ascending, for taps whose
 * even offsets other than 0 are ZERO (the Ram-Lak ramp filter): only taps[0] and the odd taps (D of them in all) are read.
 *
 * Limits: planes, H, W, A, D > 0, H, W <= AZ_OP_RADON_MAX_SIZE, D <= AZ_OP_RADON_MAX_DET, A <= AZ_OP_RADON_MAX_ANGLES, planes <=
 * 2^31, 1/8 <= inv_spacing <= 1 (else AZ_E_SHAPE).  Every pointer is required (AZ_E_NULL); images, sinograms and `work` are
 * 16-byte aligned, the table and the taps 4-byte aligned (AZ_E_ALIGN); a destination overlaps no source and not `work`, and
 * `work` no source (AZ_E_SHAPE).  table and taps are DEVICE pointers.
 *
 * az_op_radon_work: the floats of `work` of an az_op_radon_f32 call (planes H W).  Host arithmetic. */
#define AZ_OP_RADON_MAX_SIZE 1024
#define AZ_OP_RADON_MAX_DET 2048
#define AZ_OP_RADON_MAX_ANGLES 4096
int az_op_radon_f32(float* dst, const float* src, const float* table, float* work, int64_t planes, int32_t H, int32_t W, int32_t A,
                    int32_t D, float inv_spacing, az_stream_t stream);
int az_op_radon_adj_f32(float* dst, const float* src, const float* table, int64_t planes, int32_t H, int32_t W, int32_t A,
                        int32_t D, float inv_spacing, float scale, az_stream_t stream);
int az_op_radon_filter_f32(float* dst, const float* src, const float* taps, int64_t rows, int32_t D, float scale,
                           az_stream_t stream);
int az_op_radon_work(int64_t planes, int32_t H, int32_t W, int64_t* floats);

/* ---- Nonlinear measurement maps and their linearisations (csrc/nonlinear.hip; MagnitudeOperator, ClipOperator, QuantizeOperator,
 * PadOperator) -------------------------------------------------------------------------------------------------------------
 * Elementwise fp32 maps whose derivative depends on where it is taken: the linearisation entries receive the operating point (z or
 * x) again and re-read it -- the forward entries save nothing.  The cmag entries take SPLIT-complex data in az_op_fft2_f32's
 * convention: sample b of a tensor is the n floats at base + b * bstride, and the real and imaginary parts have separate bases, so
 * the two halves of a (B, 2 C, H, W) tensor are passed in place (n = C H W, bstride = 2 n).  One work item owns 4 consecutive
 * floats: bases and strides that are multiples of 4 floats with n % 4 == 0 take 16-byte loads and stores, anything else a scalar
 * form.  No atomics; a sample's result does not depend on the other samples of the launch.
 *
 * az_op_cmag_f32: y = |z|, z = re + i im, or |z|^2 (squared = 1).  With h / l the part of larger / smaller magnitude and e the
 * exponent that brings |h| into [0.5, 1): a = |h| 2^-e, b = |l| 2^-e, y = sqrt(fma(a, a, b b)) 2^e with b b rounded on its own and
 * an IEEE square root: no overflow or underflow wherever |z| is a normal number, within 2^-23 |z|, exact on integer Pythagorean
 * pairs below 2^12 at any scale.  squared: fma(re, re, im im), Inf beyond fp32's range.  A NaN part gives NaN.  12 bytes / element.
 *
 * az_op_cmag_vjp_f32: (d_re, d_im) = g u with the unit vector u = (re, im) / |z| = (re 2^-e / s, im 2^-e / s), s = |z| 2^-e as
 * above and one IEEE division per part, and exactly (0, 0) where z = 0 whatever g is: torch's sgn convention for abs of a complex
 * tensor.  squared: (2 g) re, (2 g) im, one rounding each.  20 bytes / element.
 *
 * az_op_cmag_jvp_f32: t_y = fma(u_re, t_re, u_im t_im), 0 where z = 0.  squared: 2 fma(re, t_re, im t_im).  20 bytes / element.
 *
 * az_op_clip_f32: y = min(max(gain x, lo), hi): the product rounded once, a NaN stays NaN and a zero keeps its sign -- what
 * torch.clamp(gain * x, lo, hi) gives.  8 bytes / element.
 *
 * az_op_clip_jac_f32: d = (lo <= gain x <= hi ? g : 0) gain -- bounds INCLUSIVE, 0 where x is NaN: torch.clamp's backward followed
 * by the product's.  The Jacobian is diagonal, so the entry is the vjp and the jvp.  12 bytes / element.
 *
 * az_op_quantize_f32: u = min(max(x, lo), hi), q = fadd(fmul(rint(fdiv(fsub(u, lo), step)), step), lo), every operation rounded
 * once and never fused, rint to nearest even: torch.round((torch.clamp(x, lo, hi) - lo) / step) * step + lo.  8 bytes / element.
 * Its straight-through linearisation is az_op_clip_jac_f32 with gain 1.
 *
 * az_op_pad_f32: zero padding of `planes` contiguous H x W planes to (top + H + bottom) x (left + W + right) in one launch, every
 * destination float written exactly once; adjoint = 1 is the crop, from the padded planes `src` to H x W planes `dst` (H and W
 * are the SMALL plane's in both directions).  16-byte form where W, left + W + right and left are multiples of 4.
 *
 * Limits.  cmag: B, n >= 0, n <= 2^40, strides >= 0 and, for B > 1, at least n; squared 0 or 1.  clip, quantize: n >= 0, finite
 * parameters, lo < hi, step > 0.  pad: planes, H, W, pads >= 0, each of H, W and the pads at most 2^20; adjoint 0 or 1 (else
 * AZ_E_SHAPE).  An empty tensor (B == 0 or n == 0, no destination float) launches nothing and returns AZ_OK.  Every pointer is
 * required (AZ_E_NULL) and 4-byte aligned (AZ_E_ALIGN); no destination shares a float with another destination or with a source
 * -- never in place (AZ_E_SHAPE).
 *
 * az_op_nonlinear_trip: the floats one trip of the capped grid covers (a launch of more walks the grid-stride loop again).  Host
 * arithmetic. */
int az_op_cmag_f32(float* y, int64_t y_bstride, const float* z_re, const float* z_im, int64_t z_bstride, int64_t B, int64_t n,
                   int32_t squared, az_stream_t stream);
int az_op_cmag_vjp_f32(float* d_re, float* d_im, int64_t d_bstride, const float* g, int64_t g_bstride, const float* z_re,
                       const float* z_im, int64_t z_bstride, int64_t B, int64_t n, int32_t squared, az_stream_t stream);
int az_op_cmag_jvp_f32(float* t_y, int64_t y_bstride, const float* t_re, const float* t_im, int64_t t_bstride, const float* z_re,
                       const float* z_im, int64_t z_bstride, int64_t B, int64_t n, int32_t squared, az_stream_t stream);
int az_op_clip_f32(float* y, const float* x, int64_t n, float gain, float lo, float hi, az_stream_t stream);
int az_op_clip_jac_f32(float* d, const float* g, const float* x, int64_t n, float gain, float lo, float hi, az_stream_t stream);
int az_op_quantize_f32(float* q, const float* x, int64_t n, float lo, float hi, float step, az_stream_t stream);
int az_op_pad_f32(float* dst, const float* src, int64_t planes, int64_t H, int64_t W, int32_t top, int32_t bottom, int32_t left,
                  int32_t right, int32_t adjoint, az_stream_t stream);
int az_op_nonlinear_trip(int64_t* floats);

/* ---- Twisted diffusion sampler: resample and proposal -------------------------------------------------------------
 * The non-network part of TDSSampler.step (azula/guidance/tds.py:70-102) for K particles of N elements each.
 *
 * az_tds_resample_f32 replaces tds.py:70-78: log_w = log_p (+ log_w_prev, NULL on the first step), w = softmax(log_w) and
 * ancestors[j] = min{ i : c_i > u_j } (clamped to K - 1) with c the inclusive prefix sum of w -- multinomial sampling with
 * replacement by inverse CDF on the caller's uniforms u[K] in [0, 1); it does not reproduce torch.multinomial's stream.  One
 * workgroup; maximum, sums and the CDF in fp64 in a fixed order (two runs give the same bits); 1 <= K <= 65536 (else
 * AZ_E_SHAPE).  A log-weight of -inf gives weight 0 and is never chosen.  If any log-weight is NaN or +inf, or all are -inf
 * (the reference raises inside torch.multinomial), w = NaN and ancestors[j] = j.  Pointers: natural alignment.
 *
 * az_tds_propose_f32 replaces tds.py:80-102 in one pass over five K x N streams.  With k = ancestors[j] and `coef` a DEVICE
 * pointer to [a_t, a_s, c_s = sigma_t^2 / alpha_t, k_x = sigma_s sqrt(tau) / sigma_t, scale = sigma_s sqrt(1 - tau), 1 / scale],
 * tau = (alpha_t / alpha_s * sigma_s / sigma_t)^2 (tds.py:85):
 *   m = x_hat[k] + c_s * score[k],   x_s[j] = a_s m + k_x (x_t[k] - a_t m) + scale z[j]
 *   log_w_next[j] = -sum_i (z g + g^2 / 2) - log_p[k],   g = (a_s - k_x a_t) c_s score[k] / scale
 * which is log q_s(x_s) - log q_{s|y}(x_s) - log_p[k] (tds.py:99-102) without the difference of two sums of log-densities.
 * Each term is rounded once to fp32, summed in fp32 chains of at most 5 dependent adds, then in fp64 (csrc/tds.hip); the error
 * of log_w_next is within 8 * 2^-24 * (sum_i |z g + g^2 / 2| + |log_p[k]|).  x_t, x_hat, score and log_p are NOT gathered by
 * the caller.  x_s must not overlap x_t, x_hat, score or z (AZ_E_SHAPE).  `workspace` holds K * az_tds_chunks(K, N) doubles and
 * `chunks` is that count; K <= 65536.  The K x N tensors and the workspace are 16-byte aligned.  scale == 0: x_s is the mean,
 * log_w_next is not finite.  An ancestor outside [0, K) reads nothing and gives NaN for that particle.                       */
int64_t az_tds_chunks(int64_t K, int64_t N);
int az_tds_resample_f32(const float* log_p, const float* log_w_prev, const float* u, int64_t* ancestors, float* w, int64_t K,
                        az_stream_t stream);
typedef struct AzTdsProposeArgs {
  const float* x_t;         /* (K, N), un-gathered                     */
  const float* x_hat;       /* (K, N), un-gathered                     */
  const float* score;       /* (K, N), un-gathered                     */
  const float* z;           /* (K, N) standard normal                  */
  const int64_t* ancestors; /* (K)                                     */
  const float* log_p;       /* (K), un-gathered                        */
  const float* coef;        /* DEVICE pointer, 6 floats                */
  float* x_s;               /* (K, N)                                  */
  float* log_w_next;        /* (K)                                     */
  double* workspace;        /* K * chunks doubles                      */
  int64_t K, N, chunks;
} AzTdsProposeArgs; /* 104 bytes */
int az_tds_propose_f32(const AzTdsProposeArgs* args, az_stream_t stream);

/* ---- Krylov solvers: CG and GMRES ---------------------------------------------------------------------------------
 * Replace the per-iteration tensor arithmetic of azula/linalg/solve.py; the operator calls A(.) stay with the caller.  b is
 * (rows, dim) contiguous: one independent system per row (the reference's "...i,...i" dot products reduce over the last
 * dimension only).  The state (x, r, p, V, ...) is kept in `state_dtype`, b / x0 / the operator input in `io_dtype`, the
 * operator output and r0 in `in_dtype` (0 = fp32, 1 = fp64; fp64 io requires fp64 state).  Every elementwise operation is
 * rounded separately, in the reference's order; clip(v, min=eps) passes NaN like torch.clamp.
 * Row regimes, chosen from `dim` alone: dim <= 1024 runs one wave per row and fuses each entry into one pass (reductions are
 * wave butterflies); longer rows are split into 1024-element segments, one wave each, whose partial sums go to `partial`
 * and are reduced by the next pass in a fixed order (no atomics).  The result of a row therefore never depends on the
 * number of rows or on the launch, and repeats bit for bit.  az_krylov_segments(dim) is the number of segments of a row
 * (1 in the one-wave regime); `partial` holds rows * slots * segments elements of the state dtype (CG: 2 slots, GMRES:
 * iterations + 2; unused, may be NULL, when segments == 1).  All entries are asynchronous and graph-capturable. */
#define AZ_KRYLOV_GMRES_MAX 32 /* largest GMRES `iterations` the kernels take */
int64_t az_krylov_segments(int64_t dim);

typedef struct AzCgArgs {
  const void* r0;   /* init: b, or b - A(x0) (in_dtype)                                                    */
  const void* x0;   /* init: the initial guess (io_dtype), or NULL for zeros                               */
  const void* Ap;   /* step: A(p.to(b)) (in_dtype)                                                         */
  void* x;          /* state (rows, dim)                                                                   */
  void* r;          /* state (rows, dim)                                                                   */
  void* p;          /* state (rows, dim)                                                                   */
  const void* rr;   /* step: (rows) r.r before the step                                                    */
  void* rr_out;     /* (rows) r.r after init / the step; never aliases rr                                  */
  void* p_io;       /* (rows, dim) io_dtype: p.to(b), the next operator input                              */
  void* out;        /* step: non-NULL on the last iteration, which writes x.to(b) here and nothing else    */
  void* partial;    /* long rows: 2 slots                                                                  */
  int64_t rows, dim;
  int32_t state_dtype, io_dtype, in_dtype, reserved;
} AzCgArgs; /* 120 bytes */
/* solve.py:51-61: x = x0 or 0, r = r0, rr = r.r, p = r; writes x, r, p, rr_out, p_io. */
int az_cg_init(const AzCgArgs* args, az_stream_t stream);
/* solve.py:63-73, one iteration after the caller's Ap = A(p_io): pAp -> alpha -> x, r -> rr_ -> beta -> p, p_io. */
int az_cg_step(const AzCgArgs* args, az_stream_t stream);

typedef struct AzGmresArgs {
  const void* r0;   /* init: b, or b - A(x0) (in_dtype)                                                    */
  const void* x0;   /* finish: the initial guess (io_dtype), or NULL                                       */
  const void* w;    /* arnoldi: A(V_j.to(b)) (in_dtype)                                                    */
  void* V;          /* state (iterations, rows, dim): the basis                                            */
  void* work;       /* state (rows, dim): w between the passes of long rows (unused for short rows)        */
  void* H;          /* state (rows, iterations + 1, iterations), zero-initialised by the caller            */
  void* cs;         /* state (rows, iterations)                                                            */
  void* ss;         /* state (rows, iterations)                                                            */
  void* B;          /* state (rows, iterations + 1); finish overwrites B[:iterations] with y               */
  void* v_io;       /* (rows, dim) io_dtype: V_{j+1}.to(b) (init: V_0.to(b)), the next operator input      */
  void* out;        /* finish: x.to(b) (io_dtype)                                                          */
  void* partial;    /* long rows: iterations + 2 slots                                                     */
  int64_t rows, dim;
  int32_t iterations, j;
  int32_t state_dtype, io_dtype, in_dtype, reserved;
} AzGmresArgs; /* 136 bytes */
/* solve.py:113-137: r = r0, V_0, B_0 = normalize(r); writes V_0, B[:, 0], v_io. */
int az_gmres_init(const AzGmresArgs* args, az_stream_t stream);
/* solve.py:139-166, iteration j after the caller's w = A(v_io): modified Gram-Schmidt against V_0..V_j (j + 1 dependent
 * reductions), normalize -> V_{j+1} and v_io (not on the last iteration), then the row's previous Givens rotations, the new
 * one and the B update on H / cs / ss / B. */
int az_gmres_arnoldi(const AzGmresArgs* args, az_stream_t stream);
/* solve.py:168-185: y = (H + eps I)^-1 B by back-substitution (into B), x = x0 + sum_i V_i y_i, written as x.to(b). */
int az_gmres_finish(const AzGmresArgs* args, az_stream_t stream);

/* ---- Covariance applies -------------------------------------------------------------------------------------------
 * The per-step products of azula/linalg/covariance.py (Isotropic, Diagonal, Full, DPLR, DMLR, Kronecker); the setup (from_data,
 * capacitances, the r x r eigh of inv / color, logdet) stays with the caller.  Every operand is contiguous; dtype codes are
 * 0 = fp32, 1 = fp64, and `out_dtype` must be torch's promotion of `x_dtype` and `f_dtype` (the factors' dtype); every
 * operand is converted to it on load.  Each output is one dot product (or one elementwise expression) evaluated in a fixed
 * order that depends on n and r alone, so a row's result does not depend on the number of rows and repeats bit for bit.
 * All entries are asynchronous and graph-capturable. */
#define AZ_COV_H_IDENTITY 0  /* h(e) = e                                                                 */
#define AZ_COV_H_SQRT 1      /* h(e) = sqrt(e)                                                           */
#define AZ_COV_H_INV 2       /* h(e) = 1 / e                                                             */
#define AZ_COV_H_POSTERIOR 3 /* h(e) = e / (e + rho): the spectral factor of C (C + rho I)^-1              */

typedef struct AzCovScaleArgs {
  const void* x;       /* (rows, n) x_dtype                                                                 */
  const void* e;       /* (e_len) f_dtype, e_len = n or 1 (broadcast), or NULL for h = 1                    */
  const void* u;       /* (n) f_dtype subtracted before the scale, or NULL                                 */
  const void* v;       /* (n) f_dtype added after the scale, or NULL                                       */
  const void* k_dev;   /* device scalar (scalar_dtype) multiplying x, or NULL: the host value k             */
  const void* rho_dev; /* device scalar (scalar_dtype), or NULL: the host value rho                        */
  void* y;             /* (rows, n) out_dtype; may alias x when the dtypes agree                            */
  double k, rho;
  int64_t rows, n, e_len;
  int32_t h, x_dtype, f_dtype, out_dtype, scalar_dtype, reserved;
} AzCovScaleArgs; /* 120 bytes */
/* y[b, f] = (k x[b, f] - u_f) h(e_f) + v_f. */
int az_cov_scale(const AzCovScaleArgs* args, az_stream_t stream);

typedef struct AzCovLowRankArgs {
  const void* x;     /* project: (rows, n) x_dtype; expand: the x of the diagonal term, or NULL for none    */
  const void* W;     /* (n, r) f_dtype, row-major                                                         */
  const void* c;     /* project: (n) f_dtype, or NULL for 1                                               */
  const void* a;     /* expand: (n) f_dtype, or NULL for 1                                                */
  const void* d;     /* expand: (n) f_dtype, or NULL for the constant d0                                  */
  const void* g;     /* expand: (r) f_dtype, or NULL for 1                                                */
  void* P;           /* (rows, r) out_dtype: the projection (project writes it, expand reads it)          */
  void* partial;     /* project: (az_cov_segments(n), rows, r) out_dtype; may be NULL when that is one    */
  void* y;           /* expand: (rows, n) out_dtype                                                       */
  double d0, s;      /* expand: d_f where d is NULL; the sign of the low-rank term (+1 / -1)              */
  int64_t rows, n, r;
  int32_t x_dtype, f_dtype, out_dtype, reserved;
} AzCovLowRankArgs; /* 128 bytes */
int64_t az_cov_segments(int64_t n);
/* P[b, j] = sum_f W[f, j] c_f x[b, f]; features in 512-element segments whose partial sums are reduced in a fixed order. */
int az_cov_project(const AzCovLowRankArgs* args, az_stream_t stream);
/* y[b, f] = a_f (d_f x[b, f] + s sum_j W[f, j] g_j P[b, j]).  DPLR / DMLR @: W = V, d = D, s = +1 / -1; their color:
 * W = U, a = sqrt(D), d0 = 1, g = sqrt(1 +- L) - 1; Full @ / color: W = Q, x = NULL. */
int az_cov_expand(const AzCovLowRankArgs* args, az_stream_t stream);

typedef struct AzCovModeArgs {
  const void* x;   /* (outer, n, inner) x_dtype                                                           */
  const void* Q;   /* (n, n) f_dtype, row-major                                                           */
  void* y;         /* (outer, n, inner) out_dtype; never aliases x                                        */
  int64_t outer, n, inner;
  int32_t transpose, x_dtype, f_dtype, out_dtype;
} AzCovModeArgs; /* 64 bytes */
/* One Kronecker axis: y[o, i, k] = sum_m M[i, m] x[o, m, k], M = Q (transpose = 0) or Q^T (transpose = 1). */
int az_cov_mode(const AzCovModeArgs* args, az_stream_t stream);

/* y = s * x with s read from device memory (azula/denoise.py:317 c_in * x_t, generic backbones). */
int az_scale_f32(float* y, const float* x, const float* s_dev, int64_t n, az_stream_t stream);

/* y = silu(x) = x / (1 + exp(-x)): the activation in front of every adaLN projection of the conditioning
 * vector (plugins/jit/_src/model.py:175-177,199-201), applied once so that all projections become one GEMM. */
int az_silu_f32(float* y, const float* x, int64_t n, az_stream_t stream);

/* y[r, i] = a[r*a_stride] * x[r, i] + b[r*a_stride] * z[r, i]  with a, b in device memory
 * (a_stride = 0: one scalar pair for all rows; 1: one pair per row = per-sample times t of
 * shape (B,), azula/denoise.py:306-307).  Separately rounded mul/mul/add as
 * azula/denoise.py:322  mean = c_skip * x_t + c_out * output.                               */
int az_axpby_f32(float* y, const float* a_dev, const float* x, const float* b_dev, const float* z, int64_t rows,
                 int64_t inner, int32_t a_stride, az_stream_t stream);

/* y = pos + g * (pos - neg), g in device memory: classifier-free guidance outside a fused
 * sampler (azula/guidance/cfg.py:63-65), same association and rounding as the reference.   */
int az_cfg_combine_f32(float* y, const float* pos, const float* neg, const float* g_dev, int64_t n,
                       az_stream_t stream);
/* The adjoint of that combine for a guided mean evaluated as ONE pass over the stacked batch [x_t ; x_t] (positive labels |
 * negative labels): m = (1 + g) m+ - g m-, so the cotangent of the stacked means is
 *   v2[0:n] = (1.0f + g[0]) * v,   v2[n:2n] = -g[0] * v      (in this op order; g in device memory),
 * what torch.autograd records behind azula/guidance/cfg.py:63-65 under the gradient methods of azula/guidance/dps.py:55-68 and
 * mmps.py:69-90.  Any n > 0: float4 body, scalar tail (and scalar stores to the second half when n % 4 != 0); v2 and v 16-byte
 * aligned.  The sum of the two halves of the pulled-back cotangent is az_axpby_f32.  12 B / element, HBM-bound; no time has been
 * measured for it.                                                                                                         */
int az_cfg_split_f32(float* v2, const float* v, const float* g_dev, int64_t n, az_stream_t stream);

/* ------------------------------------------------------------------ layout
 * NCHW (B,C,H,W) -> NHWC with channel stride cs (>= C, multiple of 4), scaled by *scale_dev
 * (NULL = 1).  Pad channels are written as 0.  And back.                                  */
int az_nchw_to_nhwc_f32(float* dst, const float* src, const float* scale_dev, int64_t B, int64_t C, int64_t HW,
                        int64_t cs, az_stream_t stream);
/* Nearest upsampling by an arbitrary integer factor per axis, cropped to (Hout, Wout): dst[b, y, x, :] = src[b, y / sh, x / sw, :]
 * on NHWC activations (channel stride cs).  Replaces torch.nn.Upsample(scale_factor=stride, mode="nearest") + torch.narrow of
 * azula/nn/unet.py:186,250-252 for strides that are not powers of two (those are folded into the merge convolution). */
int az_upsample_nearest_f32(float* dst, const float* src, int64_t B, int64_t Hin, int64_t Win, int64_t cs, int32_t sh,
                            int32_t sw, int64_t Hout, int64_t Wout, az_stream_t stream);

/* ------------------------------------------------------------------ v-diffusion backbones (csrc/vdm.hip)
 * az_fourier_planes_f32 replaces azula/plugins/vdm/_src/imagenet_128.py:63-75,186-189 (FourierFeatures.forward,
 * expand_to_planes and the torch.cat in front of the stem; yfcc_1.py:43-52,73-75,213-215 alike): for every pixel of the NHWC tensor
 * dst (B, HW, cs) it writes channels [c_lo, c_lo + 2 nfeat_half): cos(2 pi u w_j) for j < nfeat_half, then sin(2 pi u w_j), with
 * u = t (mode 0: the yfcc models) or u = log(cos^2(t pi / 2) / sin^2(t pi / 2)) (mode 1: _src/utils.py:51-61) and
 * t = t_dev[b * t_stride] on the DEVICE -- t_stride 0: one scalar for the batch (AzStepCoef.c_time of the current step inside a
 * captured graph), 1: one time per sample.  Every other channel is left as it is.  `weight`: nfeat_half floats.  Evaluated in
 * fp64 from the fp32 time and weights and rounded once (log(cos^2 / sin^2) is ill conditioned near t = 1; a thread evaluates its
 * features once for all its pixels): within 16 * 2^-24 * (1 + |2 pi u w|) of the exact value.  1 <= nfeat_half <= 32, cs % 4 == 0, c_lo + 2 nfeat_half <= cs, B <= 65535 (else AZ_E_SHAPE); dst 16-byte aligned.
 *
 * az_upsample_bilinear2x_f32 replaces nn.Upsample(scale_factor=2, mode="bilinear", align_corners=False) of yfcc_1.py:157-159:
 * NHWC src (B, H, W, cs) -> dst (B, 2H, 2W, cs) with ATen's taps (weights 0.25 / 0.75 per axis, 1 / 0 on the first row and
 * column, indices clamped at the far border); within 2^-22 * max |src| of the exact value.  cs % 4 == 0, dst != src, both 16-byte
 * aligned.                                                                                                                    */
int az_fourier_planes_f32(float* dst, int64_t B, int64_t HW, int64_t cs, int64_t c_lo, const float* weight, int32_t nfeat_half,
                          const float* t_dev, int64_t t_stride, int32_t mode, az_stream_t stream);
int az_upsample_bilinear2x_f32(float* dst, const float* src, int64_t B, int64_t H, int64_t W, int64_t cs, az_stream_t stream);

/* ------------------------------------------------------------------ input gradient (csrc/backward.hip)
 * The passes of a vector-Jacobian product v -> (d out / d x)^T v through the UNet that are not convolutions -- what
 * torch.autograd records behind azula/guidance/dps.py:55-68, pgdm.py:57-67, tmpd.py:55-71 and mmps.py:69-90 for the layers of
 * azula/nn/unet.py:85-95,186,250-257.  (The data gradients of the convolutions run on the az_conv2d_* entries with the weight
 * transposed and flipped.)  fp32, channel-padded NHWC (stride cs, pad lanes written as zero), deterministic: fixed-order
 * reductions, no atomics.  `scale` (NULL: none) is the modulation a of gamma = 1 + a, read at scale[b * scale_bstride + c].
 *
 * GroupNorm backward (torch.nn.GroupNorm's pullback, biased variance; azula/nn/unet.py:91): with xh = (x - mean) rstd and
 * q = gamma g,  dx = res + rstd (q - mean_group(q) - xh mean_group(q xh)).  `fpart` are the FORWARD records of
 * az_groupnorm_stats_f32 over `fchunks` pixel chunks; the stats pass writes bpart[b][chunk][group] = (sum q, sum q xh, 0, 0)
 * over `nchunks` chunks, the apply pass folds them and adds the residual `res` (NULL: none).                                  */
int az_groupnorm_bwd_stats_f32(float* bpart, const float* x, const float* g, const float* scale, int64_t scale_bstride,
                               const float* fpart, int32_t fchunks, int64_t B, int64_t HW, int64_t C, int64_t cs, int32_t groups,
                               int32_t nchunks, float eps, az_stream_t stream);
int az_groupnorm_bwd_apply_f32(float* dx, const float* x, const float* g, const float* res, const float* scale,
                               int64_t scale_bstride, const float* fpart, int32_t fchunks, const float* bpart, int32_t nchunks,
                               int64_t B, int64_t HW, int64_t C, int64_t cs, int32_t groups, float eps, az_stream_t stream);
/* Row-norm backward, one row = one pixel (azula/nn/layers.py LayerNorm with the UNBIASED variance, kind 0:
 * dx = res + rstd (q - mean(q) - xh mean(q xh) C / (C - 1)); RMSNorm, kind 1: dx = res + rstd (q - xh mean(q xh)), xh = x rstd). */
int az_rownorm_bwd_f32(float* dx, const float* x, const float* g, const float* res, const float* scale, int64_t scale_bstride,
                       int64_t rows, int64_t rows_per_batch, int64_t C, int64_t cs, int32_t kind, float eps, az_stream_t stream);
/* The same pass with a learned per-channel gain under the modulation: the pullback of y = (1 + scale[b, c]) weight[c] norm(x) + shift
 * (the RMSNorm modules of plugins/jit/_src/util.py:149-157 inside modulate(), plugins/jit/_src/model.py:175-177,199-201), i.e. the
 * formulas above with q = g weight (1 + scale).  `weight`: C floats, NULL = none -- then the launch is az_rownorm_bwd_f32's own,
 * bit for bit.  Kinds 0 and 1, same `res`, strides, zero pad lanes and determinism.  16 B / element (+ 4 B / element with `res`):
 * HBM-bound; no time has been measured for it.                                                                              */
int az_rownorm_bwd_w_f32(float* dx, const float* x, const float* g, const float* res, const float* scale, int64_t scale_bstride,
                         const float* weight, int64_t rows, int64_t rows_per_batch, int64_t C, int64_t cs, int32_t kind, float eps,
                         az_stream_t stream);
/* y = g * silu'(p), silu'(p) = s (1 + p (1 - s)), s = 1 / (1 + exp(-p)), on the PRE-activation p (the nn.SiLU between the two
 * convolutions of azula/nn/unet.py:76-83); n % 4 == 0; y may alias g.                                                        */
int az_silu_bwd_f32(float* y, const float* g, const float* p, int64_t n, az_stream_t stream);
/* y[b, p, c] = x[b, p, c] * s[b * s_bstride + c] (pad lanes zero): the gate c of out = x + c * y (azula/nn/unet.py:93) applied
 * to the cotangent; y may alias x.                                                                                            */
int az_channel_scale_f32(float* y, const float* x, const float* s, int64_t s_bstride, int64_t B, int64_t HW, int64_t C, int64_t cs,
                         az_stream_t stream);
/* FFN activations of the DiT block (azula/nn/dit.py:74-85, azula/nn/layers.py:71-110) as passes of their own -- the forward-keep
 * tape keeps the PRE-activation p -- and their pullbacks.  kind 1: silu, 2: relu, 3: relu(p)^2 (derivative 0 at p <= 0).
 * n % 4 == 0; y may alias x / g.  8 B / element forward, 12 B / element backward: HBM-bound.                                  */
int az_act_f32(float* y, const float* x, int64_t n, int32_t kind, az_stream_t stream);
int az_act_bwd_f32(float* y, const float* g, const float* p, int64_t n, int32_t kind, az_stream_t stream);
/* Pullback of az_swiglu_f32 (y[r, c] = x[r, 2c] * silu(x[r, 2c+1]), azula/nn/layers.py:107-110) on the kept pre-activation x:
 * dx[r, 2c] = g[r, c] silu(x[r, 2c+1]), dx[r, 2c+1] = g[r, c] x[r, 2c] silu'(x[r, 2c+1]); dx has x's row stride xs (lanes past
 * 2 cout written as zero), g the row stride gs.  xs % 4 == 0.  16 B per input pair: HBM-bound.                             */
int az_swiglu_bwd_f32(float* dx, const float* g, const float* x, int64_t rows, int64_t cout, int64_t xs, int64_t gs, az_stream_t stream);
/* The cotangent g (B, h, w, cs) of a convolution with stride (sh, sw) on the zero-filled (B, H, W, cs) grid of its input:
 * G[b, i sh, j sw, :] = g[b, i, j, :], zero elsewhere ((h - 1) sh <= H - 1, (w - 1) sw <= W - 1).  A stride-1 convolution of G with
 * the transposed, flipped weight is the data gradient of the strided convolution (azula/nn/unet.py:159-186).                 */
int az_zero_stuff_f32(float* G, const float* g, int64_t B, int64_t h, int64_t w, int64_t cs, int32_t sh, int32_t sw, int64_t H,
                      int64_t W, az_stream_t stream);
/* Pullback of az_upsample_nearest_f32 (Upsample(nearest) + narrow, azula/nn/unet.py:186,250-255): dx[b, i, j, :] = the sum of
 * g[b, i sh + di, j sw + dj, :] over the sh x sw window clipped to the narrowed (hn, wn) map; dx is (B, h, w, cs).            */
int az_upsample_nearest_bwd_f32(float* dx, const float* g, int64_t B, int64_t h, int64_t w, int64_t cs, int32_t sh, int32_t sw,
                                int64_t hn, int64_t wn, az_stream_t stream);

/* ------------------------------------------------------------------ input gradient of the ADM UNet (csrc/backward_adm.hip)
 * Pullback of the ADM norm pass y = pool(act(S[b,c] x + T[b,c])) -- az_groupnorm_finalize_f32's tables applied by
 * az_affine_act_f32: GroupNorm, its affine gamma / beta, FiLM (1 + scale) and shift, SiLU (act = 1) and the 2x2 (pool = 1) or 1x2
 * (pool = 2) average pool (plugins/adm/_src/unet.py:227-247) -- w.r.t. x.  With S = r_g m_c, m_c = gamma_c (1 + scale[b, c]),
 * xh = (x - mean_g) r_g and the cotangent g of y on the POOLED grid (B, H', W', cs):
 *     u = pool^T(g) act'(S x + T);  s1 = sum_group m u;  s2 = sum_group m u xh;  dx = r_g (m u - s1 / N - xh s2 / N) [+ res]
 * act' is recomputed from x, S, T: only x and the forward statistics are kept.  The input is x0 (B, H, W, cs), or the channel
 * concatenation x0 | x1 read in place as in az_groupnorm_stats_f32 (x0 of stride c0s, x1 of stride cs - c0s, C == cs; groups may
 * straddle the boundary; any C / groups); dx0 / dx1 (and the optional residuals res0 / res1 that are added) have their source's
 * layout.  `weight` = gamma (NULL: 1), `scale` read at scale[b * scale_bstride + c] (NULL: 0).  `fpart`: the forward records of
 * az_groupnorm_stats_f32 over `fchunks` chunks (mean and r_g are folded from them); the stats pass writes
 * bpart[b][chunk][group] = (s1, s2, 0, 0) over `nchunks` pixel chunks, the apply pass folds them in a fixed order.  Pad lanes
 * [C, cs) of dx0 are written as zero.  Deterministic, no atomics.                                                            */
int az_norm_affine_bwd_stats_f32(float* bpart, const float* x0, const float* x1, int64_t c0s, const float* g, const float* S,
                                 const float* T, const float* weight, const float* scale, int64_t scale_bstride, const float* fpart,
                                 int32_t fchunks, int64_t B, int64_t H, int64_t W, int64_t C, int64_t cs, int32_t groups,
                                 int32_t nchunks, int32_t act, int32_t pool, float eps, az_stream_t stream);
int az_norm_affine_bwd_apply_f32(float* dx0, float* dx1, const float* res0, const float* res1, const float* x0, const float* x1,
                                 int64_t c0s, const float* g, const float* S, const float* T, const float* weight, const float* scale,
                                 int64_t scale_bstride, const float* fpart, int32_t fchunks, const float* bpart, int32_t nchunks,
                                 int64_t B, int64_t H, int64_t W, int64_t C, int64_t cs, int32_t groups, int32_t act, int32_t pool,
                                 float eps, az_stream_t stream);
/* Pullback of the pooling-only pass (AvgPool2d(2, 2): pool = 1; AvgPool1d(2) on a one-row image: pool = 2): dx (B, H, W, cs) =
 * res + g[b, h / 2 (pool 1) or h, w / 2, :] / 4 (or / 2); g is (B, H', W', cs); res NULL: none.                                  */
int az_avgpool_bwd_f32(float* dx, const float* g, const float* res, int64_t B, int64_t H, int64_t W, int64_t cs, int32_t pool,
                       az_stream_t stream);
/* Pullback of the ADM posterior mean = clip(c_skip x_t + c_out eps, lo, hi), eps = F(c_in x_t)[:, :C] (plugins/adm/__init__.py:
 * 109-123), planar tensors: with the KEPT clipped `mean` (B, C, inner), mask = lo < mean < hi (a clipped element sits on a bound)
 * and the cotangent v of the mean,
 *   ..._out: gF (B, F, inner) = c_out mask v on the first C channels, ZERO on the other F - C (a learned log-variance does not
 *            enter the mean);
 *   ..._in : dx = c_in g + c_skip mask v, g (B, C, inner) the backbone's pullback of gF.
 * Coefficients are device scalars, or one per sample (per_sample != 0).  lo = -inf, hi = +inf: no clipping.                      */
int az_adm_precond_bwd_out_f32(float* gF, const float* v, const float* mean, const float* c_out, int32_t per_sample, int64_t B,
                               int64_t C, int64_t F, int64_t inner, float lo, float hi, az_stream_t stream);
int az_adm_precond_bwd_in_f32(float* dx, const float* g, const float* v, const float* mean, const float* c_in, const float* c_skip,
                              int32_t per_sample, int64_t B, int64_t n, float lo, float hi, az_stream_t stream);

int az_nhwc_to_nchw_f32(float* dst, const float* src, int64_t B, int64_t C, int64_t HW, int64_t cs,
                        az_stream_t stream);

/* ------------------------------------------------------------------ K5 (small M): linear + activation
 * y[m, n] = out_act( sum_k in_act(x[m, k]) * W[n, k] + bias[n] ),  M small (modulation / time MLPs:
 * azula/nn/unet.py:65-70, azula/nn/dit.py:58-63, plugins/adm/_src/unet.py:196-202,460-464).
 * act: 0 none, 1 SiLU.  K must be a multiple of 4 or K == 1.  ldy = row stride of y.        */
int az_linear_small_f32(float* y, int64_t ldy, const float* x, int64_t ldx, const float* W, const float* bias,
                        int64_t M, int64_t N, int64_t K, int32_t in_act, int32_t out_act, az_stream_t stream);
typedef struct AzLinearGroup {
  float* y;          /* (M, ldy) */
  const float* x;    /* (M, ldx); K % 4 == 0, ldx % 4 == 0, 16-byte aligned */
  const float* W;    /* (N, K) row-major, 16-byte aligned */
  const float* bias; /* (N) or NULL */
  int64_t ldy, ldx;
  int32_t N, K;
} AzLinearGroup; /* 56 bytes */
/* The same operation for `ngroups` independent (x, W, bias, y) quadruples sharing M and the activations, in ONE
 * launch: `groups_dev` is a DEVICE array of descriptors, max_n = max N over the groups.  Used to hoist all
 * per-block modulation MLPs (azula/nn/unet.py:65-70, one per UNetBlock) to the front of a forward.      */
int az_linear_small_grouped_f32(const AzLinearGroup* groups_dev, int32_t ngroups, int32_t max_n, int64_t M,
                                int32_t in_act, int32_t out_act, az_stream_t stream);

/* dst[r, :] = table[idx[r], :]  (label_emb / per-step embedding rows).  idx is int64 on device. */
int az_gather_rows_f32(float* dst, const float* table, const int64_t* idx, int64_t nrows, int64_t ncols,
                       int64_t table_rows, az_stream_t stream);
/* dst[0, :] = table[coef->time_index or coef->step, :] (which: 0 = time_index, 1 = step)       */
int az_gather_step_row_f32(float* dst, const float* table, const AzStepCoef* coef, int32_t which, int64_t ncols,
                           int64_t table_rows, az_stream_t stream);
/* dst[0] = coef->c_time (feeds the time-embedding MLP of a Karras-wrapped backbone)            */
int az_coef_c_time_f32(float* dst, const AzStepCoef* coef, az_stream_t stream);

/* ------------------------------------------------------------------ K2: GroupNorm (+ modulation, + SiLU)
 * Three launches over an NHWC tensor x (B, HW, cs):
 *  (1) az_groupnorm_stats_f32: per (b, pixel-chunk, group) partial (count, mean, M2), Chan-combinable;
 *  (2) az_groupnorm_finalize_f32: per (b, c): S = rstd*w*(1+a), T = (bias - mean*rstd*w)*(1+a) + sh
 *      so that  y = x*S + T  ==  (GN(x)*w + bias) * (1 + a) + sh
 *      (azula/nn/unet.py:91 with w=1,bias=0;  plugins/adm/_src/nn.py:87 + _src/unet.py:179-183,239-243);
 *  (3) az_affine_act_f32: y = act(x*S + T), optionally 2x2 average pooled (ADM Downsample,
 *      _src/unet.py:133).
 * partials: float[B * nchunks * groups * 4].                                                   */
/* x1 / c0s: optional second source -- the input is the channel concatenation [x (c0s) | x1 (cs - c0s)]
 * (ADM decoder: GroupNorm over cat([h, skip]), plugins/adm/_src/unet.py:631,179); NULL / 0 otherwise.  */
int az_groupnorm_stats_f32(float* partials, const float* x, const float* x1, int64_t c0s, int64_t B, int64_t HW,
                           int64_t C, int64_t cs, int32_t groups, int32_t nchunks, az_stream_t stream);
typedef struct AzNormFinalizeArgs {
  float* S;               /* (B, cs) */
  float* T;               /* (B, cs) */
  const float* partials;  /* from az_groupnorm_stats_f32 */
  const float* weight;    /* (C) or NULL (= 1) */
  const float* bias;      /* (C) or NULL (= 0) */
  const float* scale;     /* a: (C) if scale_bstride == 0 else (B, scale_bstride...) ; NULL = 0 */
  const float* shift;     /* same addressing as scale */
  int64_t scale_bstride;  /* elements between consecutive batch rows of scale/shift (0 = shared) */
  int64_t B, C, cs;
  int32_t groups, nchunks;
  float eps;
  /* partials produced by convolution epilogues (AzConvArgs.gn_quads) instead of az_groupnorm_stats_f32:
   * quads_per_group > 0 selects the layout (B, nchunks, quads, 4) with `quads0` channel quads in `partials` and, for a
   * two-source input (channel concatenation), the rest in `partials1`; group g folds quads [g qpg, (g + 1) qpg). */
  const float* partials1;
  int32_t quads_per_group, quads0;
  int32_t nchunks1;       /* partials per image in `partials1` (0 = nchunks): the two producers may chunk differently */
  int32_t reserved0;
} AzNormFinalizeArgs;
int az_groupnorm_finalize_f32(const AzNormFinalizeArgs* args, az_stream_t stream);
/* pool: 0 none, 1 = 2x2 average pool of act(.) (needs H, W even; dst is (B, H/2*W/2, cs)), 2 = 1x2 (width only: AvgPool1d(2) of
 * a signal held as a one-row image, plugins/adm/_src/nn.py:64-77 with dims = 1; dst is (B, H*W/2, cs)). */
int az_affine_act_f32(float* y, const float* x, const float* x1, int64_t c0s, const float* S, const float* T,
                      int64_t B, int64_t H, int64_t W, int64_t cs, int32_t act, int32_t pool, az_stream_t stream);

/* Row norms over the channel axis of an NHWC / token tensor (rows, cs), C real channels:
 *   kind 0: azula layer_norm, UNBIASED variance, no affine (azula/nn/layers.py:152-155);
 *   kind 1: RMS norm (azula/nn/layers.py:193-195, torch.nn.RMSNorm in azula/nn/dit.py:52-55);
 * optionally times a learned per-channel `weight` (NULL = none; the RMSNorm of the JiT plugin,
 * plugins/jit/_src/util.py:149-163), followed by y = n * (1 + a[b, c]) + sh[b, c]
 * (azula/nn/unet.py:91, azula/nn/dit.py:107, plugins/jit/_src/model.py:12-13).
 * rows_per_batch maps a row to its batch index for the modulation lookup.                      */
int az_rownorm_mod_f32(float* y, const float* x, const float* weight, const float* scale, const float* shift,
                       int64_t scale_bstride,
                       int64_t rows, int64_t rows_per_batch, int64_t C, int64_t cs, int32_t kind, float eps,
                       az_stream_t stream);
/* az_groupnorm_stats_f32 and az_affine_act_f32 on tensors held in a 2-byte type -- dtype 1: bfloat16, 2: IEEE half; x, x1 and y
 * alike: the activations of a module cast to half precision (azula/denoise.py:314-320; torch.nn.GroupNorm on a half tensor
 * computes its statistics in fp32 as well).  Strides in elements, multiples of 8; y rounded to nearest even.                  */
int az_groupnorm_stats_h16(float* partials, const void* x, const void* x1, int64_t c0s, int64_t B, int64_t HW, int64_t C,
                           int64_t cs, int32_t groups, int32_t nchunks, int32_t dtype, az_stream_t stream);
int az_affine_act_h16(void* y, const void* x, const void* x1, int64_t c0s, const float* S, const float* T, int64_t B, int64_t H,
                      int64_t W, int64_t cs, int32_t act, int32_t pool, int32_t dtype, az_stream_t stream);
/* The same on rows held in a 2-byte type -- dtype 1: bfloat16, 2: IEEE half; x and y alike: the activations of a module cast to
 * half precision (azula/denoise.py:314-320; torch's RMSNorm / the reference's layer_norm on a half tensor).  Statistics, gain and
 * modulation in fp32, output rounded to nearest even.  C % 8 == 0, C == cs, C <= 4096 (else AZ_E_UNSUPPORTED).                 */
int az_rownorm_mod_h16(void* y, const void* x, const float* weight, const float* scale, const float* shift,
                       int64_t scale_bstride, int64_t rows, int64_t rows_per_batch, int64_t C, int64_t cs, int32_t kind,
                       float eps, int32_t dtype, az_stream_t stream);

/* ------------------------------------------------------------------ K3/K5: implicit-GEMM convolution
 * out[b, oh, ow, co] = epilogue( bias[co] + sum_{ky,kx,ci} in[b, oh*s+ky-p, ow*s+kx-p, ci] * W[co, ci, ky, kx] )
 * on gfx950 fp32 MFMA (v_mfma_f32_32x32x2_f32: exact fp32 FMA chain).  Replaces
 * F.conv2d 3x3 / 1x1 (azula/nn/unet.py:79-83,175-200; plugins/adm/_src/unet.py:182,207,213,215,471,602),
 * nn.Linear on token tensors (ksize = 1: azula/nn/dit.py:88-93,169-170; azula/nn/attention.py:45-46)
 * and Conv1d k=1 (plugins/adm/_src/unet.py:277,285).
 * The input is the channel concatenation [src0 (c0) | src1 (c1)] (skip concat: azula/nn/unet.py:257,
 * plugins/adm/_src/unet.py:631); either source may be read through nearest x2 upsampling
 * (azula/nn/unet.py:187, plugins/adm/_src/unet.py:104-106) without materialising it.
 * Weights are pre-packed once as [ky*ks+kx][cout_s][cin_s] (az_pack_conv_weight_f32).
 * Epilogue: v = acc + bias; v = act(v); if (gate) v = gate[b*gate_bstride + co] * v; if (res) v += res;
 *           (azula/nn/unet.py:93 x + c*y; plugins/adm/_src/unet.py:247,296 skip + h).           */
typedef struct AzConvArgs {
  const float* src0; /* NHWC (B, h0, w0, c0s) */
  const float* src1; /* NHWC (B, h1, w1, c1s) or NULL */
  int32_t c0s, c1s;  /* channel strides (multiples of 4); input channels = c0s + c1s */
  int32_t up0, up1;  /* log2 of the nearest upsampling the source is read through (0: none, 1: x2, 2: x4, ... <= 4) */
  int32_t h0, w0, h1, w1; /* stored spatial dims of each source */
  int32_t batch, hin, win; /* logical input dims (after upsampling / narrowing) */
  const float* weight;     /* packed [ks*ks][cout_s][cin_s], cin_s = c0s + c1s */
  const float* bias;       /* (cout_s) or NULL */
  int32_t cout_s;          /* output channel stride (multiple of 4) */
  int32_t ksize, stride, pad;
  int32_t hout, wout;
  int32_t act;             /* 0 none, 1 SiLU, 2 ReLU, 3 ReLU^2, 4 SwiGLU over interleaved pairs: dst gets cout_s / 2 channels per
                              pixel, y[c] = x[2c] * silu(x[2c+1]) (no gate / res / dst_nchw; cout_s % 8 == 0), 5 q / k preparation
                              of a fused qkv projection (the qk_* fields at the end of this struct; az_conv2d_f32 family only),
                              6 SiLU of the sum with the residual: y = silu(conv + bias + res) (res required; no gate /
                              dst_nchw / gn_quads) -- the last depth tap of a Conv3d -> SiLU pair */
  const float* gate;       /* optional (…, cout_s) */
  int64_t gate_bstride;    /* 0 = shared across the batch */
  const float* res;        /* optional residual, NHWC (B, hres, wres, cout_s) */
  int32_t res_up;          /* 1: residual is read through nearest x2 upsampling (ADM up block) */
  int32_t hres, wres;
  int32_t res_bcast;       /* 1: residual is (hout, wout, cout_s), shared by the batch (positional embedding) */
  float* dst;              /* NHWC (B, hout, wout, cout_s), or NCHW (B, dst_c, hout, wout) */
  int32_t dst_nchw;        /* 1: write NCHW with dst_c real channels */
  int32_t dst_c;
  int32_t splitk;          /* >= 1; > 1 needs workspace of splitk * B*hout*wout * cout_s floats */
  float* workspace;
  int32_t pad_mode;        /* 0: zero padding; 1: circular ("periodic", azula/nn/unet.py:175-180): taps wrap around the map */
  int32_t gn_chunks;       /* with gn_quads: partials per image -- splitk 1 (az_conv2d_winograd_f32 only): tile blocks of 64 Winograd
                            * tiles; splitk > 1 (any conv entry point): chunks of ceil(hout * wout / gn_chunks) pixels */
  float* gn_quads;         /* optional: GroupNorm moments of the OUTPUT, (batch, gn_chunks, cout_s / 4, 4) floats = (n, mean, M2, 0)
                            * per image, chunk and channel quad -- from the Winograd kernel's epilogue (splitk 1, cout_s % 64 == 0,
                            * 64 | tiles per image) or from the split-K combine kernel (splitk > 1); consumed by
                            * az_groupnorm_finalize_f32 (quads_per_group), so that the normalisation that follows needs no
                            * statistics pass over the tensor */
  int32_t aniso;           /* 1: the WIDTH axis has its own stride / upsampling factors (azula/nn/unet.py:159-186 with a
                            * stride sequence such as (2, 1)); 0: `stride`, `up0`, `up1` apply to both axes.  Direct kernels
                            * (az_conv2d_f32 / _bf16_f32 / _f16_f32 / _x3_f32) only: the Winograd entries return UNSUPPORTED */
  int32_t stride_w;        /* with aniso: stride along the width (`stride` is then the height's) */
  int32_t up0_w, up1_w;    /* with aniso: log2 upsampling of each source along the width */
  const float* in_affine;  /* optional, az_conv2d_winograd_f32 only: (2, batch, c0s) floats [scale | shift]; the convolution's input
                            * is x * scale[b, c] + shift[b, c] (in_act 1: SiLU of that), evaluated on the raw patch values inside the gather --
                            * the GroupNorm apply pass that would write the normalised tensor (az_affine_act_f32) disappears.
                            * Padding stays ZERO (the reference pads the normalised tensor: azula/nn/unet.py:85-92,
                            * plugins/adm/_src/unet.py:196-203).  Needs a single source, c0s % 8 == 0, up0 == 0 */
  int32_t in_act;          /* with in_affine: 0 none, 1 SiLU */
  int32_t src_dtype;       /* az_conv2d_bf16_f32 / az_conv2d_f16_f32 only (0 elsewhere): 0 = the sources hold fp32 (rounded to the operand type
                            * per tile), 1 = they hold the launch's 2-byte operand type already -- the activations of a module cast to
                            * half precision live in HBM in the module's type (azula/denoise.py:314-320); channel strides are then
                            * multiples of 8, `src0` / `src1` are the tensors' addresses and the strides stay in ELEMENTS */
  int32_t depth;           /* > 0 (az_conv2d_f32, az_conv2d_winograd_f32; every source holds `batch` planes): the `batch` images are the planes of
                            * batch / depth volumes, and this launch is ONE DEPTH TAP of a 3-D convolution (azula/nn/layers.py:25-68
                            * with spatial = 3): image b reads source plane b + depth_shift, taken as zeros where
                            * (b % depth) + depth_shift falls outside [0, depth) -- the zero padding along the depth axis; a gate
                            * must be shared by the batch (gate_bstride 0).  The taps accumulate through `res` = `dst` */
  int32_t depth_shift;
  /* act 5 (az_conv2d_f32 and its half / x3 forms, NHWC destination, no gate / res / gn_quads, splitk 1): the output is a fused
   * q | k | v projection laid out '(3 H C)' (azula/nn/attention.py:90, plugins/jit/_src/model.py) with cout_s = 3 * qk_heads *
   * qk_head_dim, and the epilogue prepares q and k for the attention kernel ONCE -- per (token, head): RMS norm over the head's
   * channels (qk_rmsnorm 1; azula/nn/attention.py:92-93), the learned gains qk_q_weight / qk_k_weight ((head_dim) each or NULL),
   * the rotation of adjacent (re, im) channel pairs by qk_rope_cos / qk_rope_sin ((qk_tokens, qk_heads * head_dim / 2) or NULL;
   * attention.py:94-95) -- instead of every workgroup of az_attention_f32 repeating it for all keys of its head.  The v third
   * only gets the bias.  head_dim 32, 64 or 128; a pixel index is batch * qk_tokens + token. */
  int32_t qk_head_dim;
  int32_t qk_heads;
  int32_t qk_tokens;
  int32_t qk_rmsnorm;
  float qk_eps;
  int32_t qk_reserved;
  const float* qk_q_weight;
  const float* qk_k_weight;
  const float* qk_rope_cos;
  const float* qk_rope_sin;
  int32_t depth_wrap;      /* with depth: 1 = circular padding along the depth axis (azula/nn/layers.py:25-68 with
                            * padding_mode "circular": a tap that leaves the volume reads the plane at its other end) */
  int32_t dst_dtype;       /* az_conv2d_bf16_f32 / az_conv2d_f16_f32 only (0 elsewhere): 1 = `dst` AND `res` hold the launch's 2-byte operand type
                            * (rounded to nearest even on the way out; bias, activation, gate, residual arithmetic stays fp32; GroupNorm
                            * moments are those of the rounded values); the planar destination (dst_nchw) and the split-K workspace are
                            * always fp32 */
  float w_scale;           /* az_conv2d_f16x2_f32 / az_conv2d_winograd_f16x2_f32 only (ignored elsewhere): the power of two the packing
                            * (az_pack_conv_weight_f16x2_f32 / az_winograd_pack_filter_f16x2_f32) multiplied the weights by; the kernels
                            * multiply their accumulators by 1 / (activation scale * w_scale), exactly (the activation scale:
                            * AZ_F16X2_IN_SCALE, or the one derived from in_absmax0 / in_absmax1 below) */
  int32_t reserved1;
  const float* in_absmax0; /* az_conv2d_f16x2_f32 / az_conv2d_winograd_f16x2_f32 only, optional: AZ_ABSMAX_SLOTS floats written by az_absmax_f32 over */
  const float* in_absmax1; /* src0 (and src1): the kernel then scales its activation operand by the power of two that puts the LARGEST
                            * magnitude of the sources (x 4 in the Winograd form, whose V sums four pixels) into [2^13, 2^14) instead of
                            * by the fixed AZ_F16X2_IN_SCALE -- no stated range any more (any finite fp32 input), full relative precision
                            * for everything within 2^-27 of the largest value.  For inputs whose magnitude is not bounded by
                            * construction (residual / input streams).  NULL: the fixed scale.  Non-finite maxima fall back to it. */
} AzConvArgs;
/* Narrow outputs (cout_s == 4, 3x3 stride 1 pad 1, one un-upsampled source with c0s % 16 == 0: the image head of
 * azula/nn/unet.py) run a VALU kernel instead of the 128-cout MFMA tile; splitk is ignored there.              */
int az_conv2d_f32(const AzConvArgs* args, az_stream_t stream);
/* The image stem -- the network's first convolution, 3x3 / stride 1 / pad 1 over <= 4 input channels (azula/nn/unet.py:142-150
 * `UNet.in_conv`-style first layer, plugins/adm/_src/unet.py:469-471 `input_blocks[0]`) -- reading its source PLANAR, i.e. the
 * latent (batch, c0s, hin, win) exactly as azula's samplers hold it, so that no NHWC copy of the latent exists: src0 planar
 * with c0s = 1..4 channels; weight = (3, 3, c0s, cout_s) floats; bias, act 0 / 1, pad_mode, gn_quads (gn_chunks =
 * ceil(hin / 8) * ceil(win / 32)) as in az_conv2d_f32; every other option must be unset. */
int az_conv2d_stem_f32(const AzConvArgs* args, az_stream_t stream);
/* The same operation with bf16 / f16 MFMA operands (v_mfma_f32_32x32x16_{bf16,f16}, 16x the fp32 MFMA rate) and fp32
 * accumulation, for backbones cast to half precision (azula/denoise.py:314-320 casts c_in x_t to the module dtype;
 * the reference's own tolerance for that mode is tests/test_nn_unet.py:78-91).  `weight` = az_pack_conv_weight_half_f32
 * output; src / res / dst stay fp32 tensors -- activations are rounded to the operand type while they are staged.   */
int az_conv2d_bf16_f32(const AzConvArgs* args, az_stream_t stream);
int az_conv2d_f16_f32(const AzConvArgs* args, az_stream_t stream);
/* fp32 operands on the bf16 matrix pipe ("bf16x3", the default of the direct contractions since round 4; AZ_FP32_MFMA=native opts out): each fp32 value is split exactly into
 * three bf16 pieces and a product is the six largest of the nine partial products, accumulated in fp32
 * (6 x v_mfma_f32_32x32x16_bf16 per 16 channels = 0.375 x the time of 8 x v_mfma_f32_32x32x2_f32).  Error vs fp64 at the
 * level of the fp32 kernel and below the Winograd form's.  `weight` = az_pack_conv_weight_x3_f32 output; everything else
 * (fp32 src / res / dst, the fused epilogue) as az_conv2d_f32.  Same reference op: azula/nn/layers.py:48-55 ConvNd.
 * Domain: finite operands (an Inf operand splits into NaN pieces: Inf in -> NaN out, where the fp32 MFMA gives Inf); operands
 * below ~2^-110 keep ~16 significant bits (their low pieces are subnormal bf16 values).                                  */
int az_conv2d_x3_f32(const AzConvArgs* args, az_stream_t stream);
/* The split-K az_conv2d_x3_f32 wants for a filled descriptor (splitk / workspace not read): its 256 x 256-tile kernel runs one
 * workgroup per CU and splits a deep K (the 3072 -> 768 token projections) until its rounds are whole; az_conv2d_suggest_splitk's
 * value wherever the 128 x 128 kernel takes the launch.  No reference counterpart. */
int az_conv2d_x3_suggest_splitk(const AzConvArgs* args);
/* Winograd F(2x2,3x3) form of the same operation for ksize = 3, stride = 1, pad = 1: 2.25x fewer
 * multiplies in exact fp32 (transforms only add/subtract; the input transform, the 16 frequency
 * GEMMs and the output transform + epilogue are ONE kernel).  `weight` must be the host-side
 * filter transform U = G g G^T packed [chunk of 8 cin][cout block of 64][16][64][8]
 * (azula_amd/engine.py: Builder.pack_winograd); all other fields as az_conv2d_f32.             */
int az_conv2d_winograd_f32(const AzConvArgs* args, az_stream_t stream);
int az_conv2d_winograd_suggest_splitk(int64_t batch, int32_t hout, int32_t wout, int32_t cout_s, int32_t cin_s);
/* The same F(2x2,3x3) convolution with its 16 frequency GEMMs on the bf16 matrix pipe at fp32 accuracy (csrc/wino_x3.hip): U (at
 * pack time) and V = B^T d B (in the kernel) are split EXACTLY into three bf16 pieces and a product is the six largest of the
 * nine partial products on v_mfma_f32_32x32x16_bf16 with fp32 accumulation -- 0.375 x the matrix-pipe time of the fp32 form.
 * `weight` = az_winograd_pack_filter_x3_f32 output (16-channel steps; source 1 starts on a step boundary); every other field,
 * the epilogue, split-K and gn_quads as az_conv2d_winograd_f32.  Inputs are assumed finite (an Inf operand splits into NaN
 * pieces).                                                                                                                  */
int az_conv2d_winograd_x3_f32(const AzConvArgs* args, az_stream_t stream);
/* Block shape of az_conv2d_winograd_x3_f32 / az_conv2d_winograd_f16x2_f32 (host arithmetic only: no device is touched).  A
 * workgroup's 64 tiles are runs of horizontally adjacent tiles (64 x 1) or a rectangle of rect_w x rect_h tiles of one image, one
 * of 32 x 2, 16 x 4, 8 x 8, 4 x 16, which stages each pixel of its (2 rect_h + 2) x (2 rect_w + 2) window once per K step.
 * az_winograd_x3_choose_block: the launcher's choice for a (batch, hin, win) map -- the shape with the fewest staged pixel slots
 * over all blocks that needs no more blocks than the run form (`whole`: only shapes that divide the tile grid, as a launch with
 * gn_quads and splitk 1 requires) -- with that total (`slots`) and the run form's (`slots_run`).
 * az_winograd_x3_block_geometry: what block `block` of the rectangular form stages, computed by the functions the kernel's
 * prologue runs: slot_pix[512][3] = (image, row, column) of the input pixel in every staged slot ((-1, -1, -1): the slot holds
 * zeros), tile_info[64][4] = (image or -1 for a masked tile, tile row, tile column, slot of the tile's patch (0, 0); patch (r, c)
 * sits r * (2 rect_w + 2) + c slots further).  Returns the slots of the window or AZ_E_* (64 x 1 is AZ_E_UNSUPPORTED here). */
int az_winograd_x3_choose_block(int32_t batch, int32_t hin, int32_t win, int32_t whole, int32_t* rect_w, int32_t* rect_h,
                                int64_t* slots, int64_t* slots_run);
int az_winograd_x3_block_geometry(int32_t batch, int32_t hin, int32_t win, int32_t pad_mode, int32_t rect_w, int32_t rect_h,
                                  int32_t block, int32_t* slot_pix, int32_t* tile_info);
/* Structured sources of az_conv2d_winograd_x3_f32 / az_conv2d_winograd_f16x2_f32 (host arithmetic only: no device is touched, no
 * pointer of `args` is dereferenced).  A source read through nearest upsampling (up >= 1 on both axes) of an even-sized map with
 * zero or circular padding and no in_affine hands rows 1 and 2 and columns 1 and 2 of every 4 x 4 patch equal values, so 7 of its
 * 16 Winograd frequencies (xi = 2 or nu = 2) are exact zeros; on that source's K steps the kernel skips their filter loads, V
 * traffic and matrix instructions, with bit-identical outputs.  A structured src0 in front of a plain src1 counts as plain.
 * mask: bit 0 = src0, bit 1 = src1 structured by that rule; launch_mask: what a launch made now would hand the kernel (the same,
 * or 0 under AZ_DEBUG_AB=1 AZ_X3_UPS=0).                                                                                      */
int az_winograd_x3_structured_mask(const AzConvArgs* args, int32_t* mask, int32_t* launch_mask);
/* fp32 operands on the fp16 matrix pipe ("f16x2"; AZ_FP32_MFMA=f16x2): HALF the matrix instructions of the bf16x3 form.
 * An activation x enters as x' = x * AZ_F16X2_IN_SCALE = h + l / 2^11 with h = fp16(x') and l = fp16((x' - h) * 2^11) (22 - 23
 * significant bits), a weight as w' = w * w_scale = wh + wl (two fp16 pieces, the residual unscaled) plus a third plane
 * whs = wh / 2^11, and a product is THREE partial products on v_mfma_f32_32x32x16_f16 with fp32 accumulation in ONE accumulator,
 *      wh h + wl h + whs l  =  w' x' - wl (x' - h)      (the dropped term is <= 2^-22 |w' x'|),
 * scaled back by 1 / (AZ_F16X2_IN_SCALE * w_scale) (powers of two: exact) before the fused epilogue.  Measured against fp64 the
 * result is as accurate as the fp32 MFMA kernel (the fp32 accumulation dominates both; tests/test_gpu_kernels.py::
 * test_conv2d_x3_accuracy).  The gfx950 matrix pipe honours fp16 subnormals (tools/mfma_denorm_probe.hip), so the pieces degrade
 * gracefully at the small end.  DOMAIN (stated, unlike bf16x3's, which is all of fp32): |x| * AZ_F16X2_IN_SCALE < 65520 --
 * activations up to ~1.0e6 (Winograd form: 4-pixel sums of the input, i.e. inputs up to ~2.6e5); beyond it a piece is Inf and the
 * outputs that depend on it are NaN (never a silently wrong finite value).  At the small end every operand carries an absolute
 * error <= 2^-36 / AZ_F16X2_IN_SCALE = 2.3e-10 (full relative precision from |x| >= 1e-3 on).  The host takes that fixed range
 * only for the DIRECT output of a normalisation: a modulated norm is bounded by |1 + a| sqrt(n) + |b| per element (n = the
 * channels / group size it averages over), a limit that remains in force and is not checked per step.  The output of a
 * convolution or attention is never taken on the fixed scale, whatever its inputs: its magnitude is set by the weights.  For
 * every other input pass the sources' largest magnitude (in_absmax0 / in_absmax1, from az_absmax_f32 or bounded from the
 * producer's moments by az_absmax_from_moments_f32) and the kernel picks the scale itself: no stated range.  bf16x3 stays selectable
 * (AZ_FP32_MFMA=bf16x3).  `weight` = az_pack_conv_weight_f16x2_f32 / az_winograd_pack_filter_f16x2_f32 output (the layouts of the x3
 * packings: three 2-byte planes), `w_scale` the scale given to that packing; everything else as the x3 entries.  Same reference
 * op: azula/nn/layers.py:25-68 ConvNd / torch.nn.Linear on tokens (azula/nn/dit.py:88-93, azula/nn/attention.py:45-46). */
#define AZ_F16X2_IN_SCALE 0.0625f
int az_conv2d_f16x2_f32(const AzConvArgs* args, az_stream_t stream);
int az_conv2d_winograd_f16x2_f32(const AzConvArgs* args, az_stream_t stream);
/* The weight scale the f16x2 packings want for a weight tensor whose largest magnitude is `amax`: the power of two that puts
 * amax (times 2.25 for the Winograd transform G g G^T when `winograd`) into (2^13, 2^14]; 1 for amax = 0 / non-finite. */
float az_f16x2_weight_scale(float amax, int32_t winograd);
/* slots[i] = max |x| over the elements workgroup i visits, i < AZ_ABSMAX_SLOTS (every slot is written: no initialisation, no
 * atomics, deterministic): the largest magnitude of an activation tensor for AzConvArgs.in_absmax0 / in_absmax1.  One streaming
 * read of the tensor (HBM-bound).  NaN elements are ignored (they turn the outputs they reach into NaN through their own pieces). */
#define AZ_ABSMAX_SLOTS 256
int az_absmax_f32(float* slots, const float* x, int64_t n, az_stream_t stream);
/* The same slots WITHOUT reading the tensor, from the GroupNorm partial moments its producing convolution left (AzConvArgs.gn_quads:
 * `count` records of (n, mean, M2, -)): every element of a record satisfies |x| <= |mean| + sqrt(M2), so the slots hold an UPPER
 * bound of max |x| (loose by up to sqrt(n): a few binades of the f16x2 pieces' 30, no precision).  NaN moments are ignored. */
int az_absmax_from_moments_f32(float* slots, const float* partials, int64_t count, az_stream_t stream);
/* Winograd F(4x4,3x3) form (6x6 patches, 36 frequency GEMMs: 2.25 multiplies per output instead of 4 / 9).
 * NOT exact: the transforms multiply by 2, 4, 5, 8 and the filter transform by 1/4 .. 1/24, so the fp32
 * rounding error is ~20x that of the F(2x2) kernel (~1e-5 of the output scale per layer).  Opt-in
 * (AZ_WINOGRAD=4).  `weight` = az_winograd4_pack_filter_f32 output; other fields as az_conv2d_f32.  */
int az_conv2d_winograd4_f32(const AzConvArgs* args, az_stream_t stream);
int az_conv2d_winograd4_suggest_splitk(int64_t batch, int32_t hout, int32_t wout, int32_t cout_s, int32_t cin_s);
/* Suggested split-K factor for a conv shape on this device (pure function of the shape).     */
int az_conv2d_suggest_splitk(int64_t npix, int32_t cout_s, int32_t cin_s, int32_t ksize);
/* torch layout (cout, cin, ks, ks) -> packed [ks*ks][cout_s][cin_s] with zero padding; the
 * input channels [0, cin0) map to packed [0, cin0) and [cin0, cin) to [c0s, c0s + cin - cin0)
 * (two-source concat with padded strides).  Runs on the device.                               */
int az_pack_conv_weight_f32(float* dst, const float* src, int32_t cout, int32_t cin, int32_t ks, int32_t cout_s,
                            int32_t cin0, int32_t c0s, int32_t cin_s, az_stream_t stream);

/* ------------------------------------------------------------------ K4: multi-head self-attention
 * out[b, t, h, :] = softmax_s( scale * <q[b,t,h,:], k[b,s,h,:]> ) v[b,s,h,:], fp32 softmax, flash-style.
 * Element (b, t, h, c) of q is at q + b*q_bstride + t*q_tstride + h*q_hstride + c (c contiguous);
 * likewise k, v, out -- so one kernel serves the fused-QKV layouts of
 *   azula/nn/attention.py:89-104   '(n H C)' + per-head q/k RMSNorm (qk_rmsnorm = 1) + SDPA (scale = C^-1/2),
 *   plugins/adm/_src/unet.py:338-345  legacy '(H 3 C)' order, scale = C^-1/4 on q and k (pass C^-1/2),
 *   plugins/adm/_src/unet.py:371-379  new '(3 H C)' order,
 *   plugins/jit/_src/model.py:121-142  '(3 H C)' + weighted q/k RMSNorm + 2-D rotary + SDPA.
 * head_dim in {8 (fp32 only), 16, 32, 64, 80, 128} (80 = JiT-H); all strides multiples of 4 floats.                 */
typedef struct AzAttnArgs {
  const float* q;
  const float* k;
  const float* v;
  float* out;
  int32_t batch, heads, tokens, head_dim;
  int64_t q_bstride, q_tstride, q_hstride;
  int64_t k_bstride, k_tstride, k_hstride;
  int64_t v_bstride, v_tstride, v_hstride;
  int64_t o_bstride, o_tstride, o_hstride;
  float scale;
  int32_t qk_rmsnorm; /* 1: q and k rows are RMS-normalised (eps) before the dot product */
  float eps;
  /* channels the RMS norm averages over; 0 = head_dim.  The kernels exist for head_dim 16 / 32 / 64 / 80 / 128 (fp32: also 8):
   * the host runs any other head size d (azula/nn/attention.py:35-51 accepts every channels // attention_heads) by zero-padding
   * each head of q, k, v to the next instantiated size when it packs the projections -- zero channels change neither q.k nor
   * p.v -- and passes norm_dim = d here (scale is explicit: 1 / sqrt(d) of the REAL size).                                  */
  int32_t norm_dim;
  /* optional rotary embedding (azula/nn/attention.py:93-96,112-156): cos/sin of theta, laid out
   * (tokens, heads, head_dim / 2), shared by the batch; adjacent channel pairs (2i, 2i+1) of q and k are
   * rotated after the RMS norm.  NULL = no RoPE.                                                */
  const float* rope_cos;
  const float* rope_sin;
  /* optional learned gains (head_dim floats, shared by all heads) applied to the RMS-normalised q / k
   * before the rotation (plugins/jit/_src/model.py:108-109,129-133).  NULL = no gain.          */
  const float* q_weight;
  const float* k_weight;
  /* optional boolean attention mask (azula/nn/attention.py:72-104 -> scaled_dot_product_attention(attn_mask=mask)):
   * one byte per (query, key) pair, non-zero = the query may attend to the key; laid out (tokens, tokens) with a batch
   * and a head stride in bytes (0 = shared by all samples / heads).  A query whose keys are all masked yields NaN, as
   * in the reference (its whole output row, and only that row); key tiles that are entirely masked for a query, before
   * or after its first live key, contribute nothing.  Both behaviours and strides other than 0 are pinned by
   * tests/test_gpu_attention.py.  NULL = no mask.                                                                  */
  const uint8_t* mask;
  int64_t mask_bstride, mask_hstride;
  /* az_attention_bf16_f32 / az_attention_f16_f32 only (0 elsewhere): 1 = q, k, v and out hold the entry's 2-byte type (the
   * activations of a module cast to half precision live in HBM in the module's type); strides stay in ELEMENTS, addresses and
   * strides need 8-byte granularity.  Norms, gains, RoPE and the softmax stay fp32.                                      */
  int32_t io_dtype;
  int32_t reserved;
} AzAttnArgs;
int az_attention_f32(const AzAttnArgs* args, az_stream_t stream);
/* The same operation for backbones cast to half precision: q / k / v / out stay fp32 tensors, norms, gains, RoPE and the
 * online softmax stay fp32, both contractions run on v_mfma_f32_32x32x16_{bf16,f16} (fp32 accumulate); exp via exp2. */
/* az_attention_f32's arithmetic on the bf16 matrix pipe at fp32 accuracy: q, k, v and the probabilities are split exactly into
 * three bf16 pieces and each product is six partial products on v_mfma_f32_32x32x16_bf16 with fp32 accumulation (softmax, norms,
 * RoPE in fp32); the attention of fp32 modules when AZ_FP32_MFMA = bf16x3 (the default).  head_dim 16, 32, 64, 80, 128.
 * Replaces the same reference lines as az_attention_f32. */
int az_attention_x3_f32(const AzAttnArgs* args, az_stream_t stream);
/* The same kernel in the f16x2 form (see az_conv2d_f16x2_f32): three partial products per contraction on v_mfma_f32_32x32x16_f16 --
 * the keys as [kh | kl | kh / 2^11] of k * 2^4 and the queries as [h | l] of q / 2^4 (the scales cancel); the probabilities (at most
 * 2^8 under the lazy running maximum) as three pieces of p * 2^6, the values as two of v / 2^4 (1 / 4 folded into the final 1 / l).
 * Softmax, norms, gains, RoPE in fp32 as before.  Domain: |k| < 4094, |v| and |q * scale * log2 e| < 1.0e6 (beyond: NaN).  The
 * host takes this entry only for RMS-normalised q / k (in the kernel or the projection epilogue), whose elements are bounded by
 * sqrt(d) max |gain| -- checked at plan time against half of these limits; un-normalised keys run az_attention_x3_f32 (all of
 * fp32).  There is no dynamic scale for v: |v| < 1.0e6 remains a stated limit.  Same reference op: torch SDPA behind
 * azula/nn/attention.py:89-104, plugins/adm/_src/unet.py:338-379.                                                       */
int az_attention_f16x2_f32(const AzAttnArgs* args, az_stream_t stream);
int az_attention_bf16_f32(const AzAttnArgs* args, az_stream_t stream);
int az_attention_f16_f32(const AzAttnArgs* args, az_stream_t stream);

/* ------------------------------------------------------------------ attention input gradient (csrc/attention_bwd.hip)
 * The pullback torch.autograd records behind azula/nn/attention.py:89-108,112-156 (per-head q / k RMSNorm, RoPE,
 * scaled_dot_product_attention), in three entries.  All fp32; all strides multiples of 4 floats, pointers 16-byte aligned;
 * head_dim in {16, 32, 64, 128} (else AZ_E_UNSUPPORTED; other sizes run zero-padded to the next of these, norm_dim = the real size).
 *
 * az_qk_prep_f32 (forward-keep side): q^ = rope(rms_norm(q)), k^ = rope(rms_norm(k)) out of place, from the fused q | k | v token
 * tensor (element (b, t, h, c) at b * in_bstride + t * in_tstride + h * in_hstride + c) into a second buffer (out_* strides).
 * rms_norm averages over norm_dim channels (0 = head_dim) with eps; qk_rmsnorm = 0: no norm.  rope_cos / rope_sin: the
 * (tokens, heads, head_dim / 2) tables of AzAttnArgs; NULL = no rotation.  The forward attention entries then run on (q^, k^, v)
 * with qk_rmsnorm = 0 and no tables.  One row per D / 4 lanes; 8 B / element: HBM-bound.                                    */
int az_qk_prep_f32(float* q_hat, float* k_hat, const float* q, const float* k, int64_t batch, int64_t tokens, int32_t heads,
                   int32_t head_dim, int64_t in_bstride, int64_t in_tstride, int64_t in_hstride, int64_t out_bstride,
                   int64_t out_tstride, int64_t out_hstride, int32_t qk_rmsnorm, int32_t norm_dim, float eps, const float* rope_cos,
                   const float* rope_sin, az_stream_t stream);
/* Its pullback: the rotation's transpose (pairs (2i, 2i+1) turned by -theta) on dq^ / dk^ (g_* strides), then the RMS-norm
 * pullback per head row, dx = r (g - xh mean(g xh)), r = rsqrt(mean(x^2) + eps) recomputed from the kept raw q / k (in_* strides),
 * means over norm_dim; writes the q and k thirds of the dqkv token tensor (out_* strides).  12 B / element: HBM-bound.   */
int az_qk_prep_bwd_f32(float* dq, float* dk, const float* dq_hat, const float* dk_hat, const float* q, const float* k, int64_t batch,
                       int64_t tokens, int32_t heads, int32_t head_dim, int64_t g_bstride, int64_t g_tstride, int64_t g_hstride,
                       int64_t in_bstride, int64_t in_tstride, int64_t in_hstride, int64_t out_bstride, int64_t out_tstride,
                       int64_t out_hstride, int32_t qk_rmsnorm, int32_t norm_dim, float eps, const float* rope_cos,
                       const float* rope_sin, az_stream_t stream);
/* The same pair with learned gains between the RMS norm and the rotation (q_norm.weight / k_norm.weight of
 * plugins/jit/_src/model.py:112-134 with plugins/jit/_src/util.py:100-157): forward q^ = rope(w_q rms_norm(q)); backward
 * u = R^T g, qg = w u, dx = r (qg - xh mean(qg xh)), xh = x r, means over norm_dim, r recomputed from the kept raw q / k.
 * q_weight / k_weight: head_dim floats each, 16-byte aligned, NULL = gain 1; zero-padded heads carry gain 1 (and cos 1, sin 0) on
 * the pad lanes.  With both NULL the launches are those of the entries above, bit for bit.  8 B / element forward, 12 B /
 * element backward (+ tables and gains): HBM-bound; no time has been measured for them.                                  */
int az_qk_prep_w_f32(float* q_hat, float* k_hat, const float* q, const float* k, int64_t batch, int64_t tokens, int32_t heads,
                     int32_t head_dim, int64_t in_bstride, int64_t in_tstride, int64_t in_hstride, int64_t out_bstride,
                     int64_t out_tstride, int64_t out_hstride, int32_t qk_rmsnorm, int32_t norm_dim, float eps, const float* rope_cos,
                     const float* rope_sin, const float* q_weight, const float* k_weight, az_stream_t stream);
int az_qk_prep_bwd_w_f32(float* dq, float* dk, const float* dq_hat, const float* dk_hat, const float* q, const float* k, int64_t batch,
                         int64_t tokens, int32_t heads, int32_t head_dim, int64_t g_bstride, int64_t g_tstride, int64_t g_hstride,
                         int64_t in_bstride, int64_t in_tstride, int64_t in_hstride, int64_t out_bstride, int64_t out_tstride,
                         int64_t out_hstride, int32_t qk_rmsnorm, int32_t norm_dim, float eps, const float* rope_cos,
                         const float* rope_sin, const float* q_weight, const float* k_weight, az_stream_t stream);
/* az_attention_bwd_f32: with P = softmax(scale q^ k^T + mask), out = P v and dout the cotangent of out,
 *   Delta_t = sum_c dout_tc out_tc,  dv = P^T dout,  dP = dout v^T,  dS = P o (dP - Delta),  dq^ = scale dS k^,  dk^ = scale dS^T q^.
 * Three launches: row statistics (the log-sum-exp is recomputed by online softmax -- the forward entries do not export it -- and
 * Delta) into `workspace` (2 * batch * heads * tokens floats), then dk^ / dv (a wave owns 32 keys and walks the queries), then dq^
 * (a wave owns 32 queries and walks the keys).  Eight contractions (8 * 2 * tokens^2 * head_dim FLOP per (batch, head) against the
 * forward's 2 * 2 * ...), on v_mfma_f32_32x32x2_f32 with fp32 accumulation; exp via exp2 in fp32; P is never stored.
 * Expected to be matrix-pipe bound (not measured).  Deterministic: no atomics, every element summed by one wave in a fixed order and stored once.  No tensor
 * takes a half-precision form (a cotangent has no range).  `mask` as in AzAttnArgs: masked pairs contribute exactly zero, tiles
 * without a live pair are skipped; a query without a live key is outside the contract (the forward is NaN there).  The outputs
 * must not overlap the inputs.                                                                                             */
typedef struct AzAttnBwdArgs {
  const float* q; /* q^ */
  const float* k; /* k^ */
  const float* v;
  const float* out;
  const float* dout;
  float* dq;
  float* dk;
  float* dv;
  float* workspace;
  const uint8_t* mask;
  int64_t mask_bstride, mask_hstride;
  int32_t batch, heads, tokens, head_dim;
  int64_t q_bstride, q_tstride, q_hstride;
  int64_t k_bstride, k_tstride, k_hstride;
  int64_t v_bstride, v_tstride, v_hstride;
  int64_t o_bstride, o_tstride, o_hstride;
  int64_t do_bstride, do_tstride, do_hstride;
  int64_t dq_bstride, dq_tstride, dq_hstride;
  int64_t dk_bstride, dk_tstride, dk_hstride;
  int64_t dv_bstride, dv_tstride, dv_hstride;
  float scale;
  int32_t reserved;
} AzAttnBwdArgs;
int az_attention_bwd_f32(const AzAttnBwdArgs* args, az_stream_t stream);

/* y[r, c] = x[r, 2c] * silu(x[r, 2c+1]), c < cout (SwiGLU, azula/nn/layers.py:89-110); xs / ys = row strides.  The (value, gate)
 * pairs are read as 8-byte vectors: xs % 2 == 0 (AZ_E_SHAPE), x 8-byte aligned (AZ_E_ALIGN).  Lanes cout .. ys of y are zeroed. */
int az_swiglu_f32(float* y, const float* x, int64_t rows, int64_t cout, int64_t xs, int64_t ys, az_stream_t stream);

/* Token-window helpers for sequences that grow / shrink inside a backbone (JiT in-context class
 * tokens, plugins/jit/_src/model.py:362-374).  Token tensors are (B, tokens, cs), cs % 4 == 0.
 *   copy: dst[b, dst_off + i, :] = src[b, src_off + i, :]            i < n   (torch.cat / x[:, k:])
 *   fill: dst[b, dst_off + j, :] = row[b * row_bstride + :] + pos[j, :]  j < n
 *         (y_emb.unsqueeze(1).repeat(1, n, 1) + in_context_posemb)                                 */
int az_token_copy_f32(float* dst, int64_t dst_tokens, int64_t dst_off, const float* src, int64_t src_tokens,
                      int64_t src_off, int64_t n, int64_t B, int64_t cs, az_stream_t stream);
int az_token_fill_f32(float* dst, int64_t dst_tokens, int64_t dst_off, int64_t n, const float* row,
                      int64_t row_bstride, const float* pos, int64_t B, int64_t cs, az_stream_t stream);
/* fill with the DESTINATION in a 2-byte type (dtype 1: bfloat16, 2: IEEE half; row / pos fp32; cs % 8 == 0): the class tokens of a
 * module cast to half precision whose activations live in HBM in its own type.  (A copy between two such tensors is
 * az_token_copy_f32 with cs / 2: two 2-byte values per float.)                                                              */
int az_token_fill_h16(void* dst, int64_t dst_tokens, int64_t dst_off, int64_t n, const float* row, int64_t row_bstride,
                      const float* pos, int64_t B, int64_t cs, int32_t dtype, az_stream_t stream);

/* Sinusoidal timestep embedding (plugins/jit/_src/model.py:59-81): dst[r, 0:half] = cos(t_r f),
 * dst[r, half:2 half] = sin(t_r f), f_j = exp(-ln(max_period) j / half); t_r = t_dev[r * t_stride]
 * (t_stride 0: one device scalar, e.g. AzStepCoef.c_time of the current step).                     */
int az_timestep_embedding_f32(float* dst, int64_t ldd, const float* t_dev, int64_t t_stride, int64_t rows,
                              int32_t half, float max_period, az_stream_t stream);

/* Patchify NCHW (B, Z, H, W) -> tokens (B, H/p * W/p, cs), feature = z*p*p + a*p + b, scaled by
 * *scale_dev (NULL = 1), pad features zero; and back (azula/nn/layers.py:198-247, azula/nn/vit.py:92-106). */
int az_patchify_f32(float* dst, const float* src, const float* scale_dev, int64_t B, int64_t Z, int64_t H, int64_t W,
                    int64_t p, int64_t cs, az_stream_t stream);
int az_unpatchify_f32(float* dst, const float* src, int64_t B, int64_t Z, int64_t H, int64_t W, int64_t p, int64_t cs,
                      az_stream_t stream);

/* az_pack_conv_weight_f32's layout in 2-byte elements (f16 != 0: IEEE half, else bfloat16; round to nearest even). */
int az_pack_conv_weight_half_f32(void* dst, const float* src, int32_t cout, int32_t cin, int32_t ks, int32_t cout_s,
                                 int32_t cin0, int32_t c0s, int32_t cin_s, int32_t f16, az_stream_t stream);
/* The same layout as three bf16 planes [piece][tap][cout_s][cin_s] with w = w1 + w2 + w3 exactly (az_conv2d_x3_f32);
 * dst holds 3 * ks*ks*cout_s*cin_s two-byte elements.                                                              */
int az_pack_conv_weight_x3_f32(void* dst, const float* src, int32_t cout, int32_t cin, int32_t ks, int32_t cout_s,
                               int32_t cin0, int32_t c0s, int32_t cin_s, az_stream_t stream);
/* The same three-plane layout for az_conv2d_f16x2_f32: planes [wh | wl | wh / 2^11] of w' = w * w_scale as IEEE half values
 * (wh = fp16(w'), wl = fp16(w' - wh)); w_scale = az_f16x2_weight_scale(max |w|, 0) (a power of two).                    */
int az_pack_conv_weight_f16x2_f32(void* dst, const float* src, int32_t cout, int32_t cin, int32_t ks, int32_t cout_s,
                                  int32_t cin0, int32_t c0s, int32_t cin_s, float w_scale, az_stream_t stream);

/* torch (cout, cin, 3, 3) -> Winograd filter transform U = G g G^T (fp64 accumulate, one rounding) in
 * the layout az_conv2d_winograd_f32 streams: [nk chunks of 8 cin][cblocks of 64 cout][16][64][8]; input
 * channels [0, cin0) fill chunks [0, nk0), the rest start at chunk nk0 (two-source concat).      */
int az_winograd_pack_filter_f32(float* dst, const float* src, int32_t cout, int32_t cin, int32_t cin0, int32_t nk0,
                                int32_t nk, int32_t cblocks, az_stream_t stream);

/* The same transform for az_conv2d_winograd_x3_f32: U (rounded to fp32 as above) split exactly into three bf16 pieces, in the
 * order that kernel's waves load it as MFMA A fragments: [nk steps of 16 cin][cblocks of 64 cout][wave 0..7 = k * 4 + frequency
 * row xi][f: nu = k + 2 f][32-cout half][piece][lane][8 bf16] (96 KB per step and cout block; opaque to callers).  dst holds
 * nk * cblocks * 49152 two-byte elements; channels [0, cin0) fill steps [0, nk0), the rest start at step nk0.      */
int az_winograd_pack_filter_x3_f32(void* dst, const float* src, int32_t cout, int32_t cin, int32_t cin0, int32_t nk0,
                                   int32_t nk, int32_t cblocks, az_stream_t stream);
/* The same fragment-ordered layout for az_conv2d_winograd_f16x2_f32: the three 2-byte pieces of an element are
 * [uh | ul | uh / 2^11] of u' = U * w_scale (IEEE half), w_scale = az_f16x2_weight_scale(max |g|, 1).                    */
int az_winograd_pack_filter_f16x2_f32(void* dst, const float* src, int32_t cout, int32_t cin, int32_t cin0, int32_t nk0,
                                      int32_t nk, int32_t cblocks, float w_scale, az_stream_t stream);

/* Same for F(4x4,3x3) (points 0, +-1, +-2, inf): [nk chunks of 4 cin][cblocks of 64 cout][36][64][4]; packed
 * channel position pc maps to input channel pc (pc < cin0) or cin0 + pc - c0s (pc >= c0s).        */
int az_winograd4_pack_filter_f32(float* dst, const float* src, int32_t cout, int32_t cin, int32_t cin0, int32_t c0s,
                                 int32_t nk, int32_t cblocks, az_stream_t stream);

/* ------------------------------------------------------------------ hipGraph helpers (host side)
 * Capture everything enqueued on `stream` between begin/end into an executable graph.         */
typedef struct AzGraph AzGraph;
int az_graph_begin(az_stream_t stream);
int az_graph_end(az_stream_t stream, AzGraph** out);
int az_graph_launch(AzGraph* g, az_stream_t stream);
int az_graph_destroy(AzGraph* g);
int az_graph_num_nodes(AzGraph* g, int64_t* n);

/* ------------------------------------------------------------------ fp64 latents
 * `Sampler(dtype=torch.float64)`: the reference's schedule scalars become fp64 tensors of shape (1, ..., 1) and promote
 * the latents to fp64 in the preconditioning (azula/denoise.py:306-322) and in every sampler update
 * (azula/sample.py:210-214, 257-259, 296-303, 343-350, 417-431, 975-993), while the backbone keeps its dtype.
 *   az_transition_f64:   the flat form of az_transition_f32 on fp64 tensors (x_t, F = posterior mean or backbone output,
 *                        eps, x_s, mean_out are double*; `coef` points to 12 doubles in AzStepCoef's field order)
 *   az_axpby_f64:        y = a x + b z, fp64, z read as float (z_is_f32) or double; a, b device scalars or per-row
 *   az_scale_f64_to_f32: y = (float)(s x)   -- `(c_in * x_t).to(backbone dtype)`, azula/denoise.py:317                */
int az_transition_f64(const AzTransitionArgs* args, az_stream_t stream);
/* Captured loop with fp64 latents (round 4): cur[0, words) = table[*step_counter - 1][0, words) -- the fp64 coefficients of the
 * step az_step_begin has just started (the fp32 row feeds the backbone's time embedding, this one az_scale_f64_to_f32 /
 * az_axpby_f64 / az_transition_f64 through pointers into `cur`), so that ONE graph serves every step.  words <= 64. */
int az_step_row_f64(double* cur, const double* table, const int32_t* step_counter, int32_t n_rows, int32_t words,
                    az_stream_t stream);
int az_axpby_f64(double* y, const double* a_dev, const double* x, const double* b_dev, const void* z, int32_t z_is_f32,
                 int64_t rows, int64_t inner, int32_t a_stride, az_stream_t stream);
int az_scale_f64_to_f32(float* y, const double* x, const double* s_dev, int64_t rows, int64_t inner, int32_t s_stride,
                        az_stream_t stream);

/* ------------------------------------------------------------------ multi-GPU sampling (no reference counterpart:
 * the reference draws `torch.randn_like(x_t)` of the whole batch on one device, azula/sample.py:214,259)
 * dst[e] = element start + e of the standard-normal tensor that torch.randn / Tensor.normal_ (float32) would draw with the
 * Philox state (seed, offset) in a launch of `threads_total` threads (ATen's policy: 256 x min(ceil(numel / 256),
 * CUs x max resident threads / 256)) -- bit for bit, so that a rank of a batch-sharded run draws only ITS samples of the
 * single-device random stream.  The caller advances the generator's offset as the full draw would.                        */
int az_randn_slice_f32(float* dst, uint64_t seed, uint64_t offset, int64_t threads_total, int64_t start, int64_t count,
                       az_stream_t stream);

/* ------------------------------------------------------------------ measurement support (not on the sampling path)
 * Known-traffic kernels that calibrate the rocprofv3 FETCH_SIZE / WRITE_SIZE counters on gfx950 (MI355X_MICROARCH.md,
 * section HBM: "calibrate on a known byte count in your own access pattern").  `az_calib_read_f32` reads every byte of
 * `src[0, nbytes)` exactly once: the buffer is rows of `row_bytes`, each read as sectors of `group_bytes` contiguous
 * bytes by `group_bytes / width` adjacent lanes (`width` = 8 or 16 bytes per lane), the sectors of a row by consecutive
 * instructions.  `az_calib_write_f32` fills `dst[0, nbytes)` with 16-byte-per-lane stores.  The reference has no
 * counterpart (it has no native code); used by tools/pmc_traffic.py and bench.py's roofline leg only.               */
int az_calib_read_f32(const float* src, float* sink, int64_t nbytes, int32_t width, int32_t group_bytes,
                      int64_t row_bytes, az_stream_t stream);
int az_calib_write_f32(float* dst, int64_t nbytes, float value, az_stream_t stream);
/* `workgroups` x 4 waves, each issuing iters x 8 independent v_mfma_f32_32x32x2_f32 on registers (4096 FLOP each): the fp32
 * MFMA rate the chip SUSTAINS under its power limit, which bench.py reports beside the nominal 157.3 TF/s peak. */
int az_calib_mfma_f32(float* sink, int32_t workgroups, int32_t iters, float a, float b, az_stream_t stream);
/* The same instruction stream on per-lane PSEUDO-RANDOM operands (uniform in [-a, a) x [-b, b), a different pair per
 * accumulator chain).  `az_calib_mfma_f32` multiplies the same two constants forever, which toggles almost nothing (~690 W on
 * MI355X); on random bit patterns the matrix pipe alone draws what a real GEMM's does, and the 1400 W cap -- not the 2.4 GHz
 * clock -- sets the rate (tools/power_probe.py).  bench.py reports both as the context of `roofline.frac`. */
int az_calib_mfma_random_f32(float* sink, int32_t workgroups, int32_t iters, float a, float b, az_stream_t stream);
/* The bf16 pipe: 8 independent v_mfma_f32_32x32x16_bf16 per iteration (32768 FLOP each) on per-lane random bf16 operands:
 * the rate the power cap leaves the instruction of the bf16x3 kernels (nominal 2516.8 TF/s). */
int az_calib_mfma_random_bf16(float* sink, int32_t workgroups, int32_t iters, float a, float b, az_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* AZULA_AMD_H */
