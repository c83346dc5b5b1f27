// Input-gradient (vector-Jacobian product) kernels of the UNet on the channel-padded NHWC layout.  All fp32, all HBM-bound.
//
// The heavy part of a pullback -- the data gradients of the convolutions -- runs on the forward convolution kernels with the
// weight transposed and flipped (engine.Builder.conv_dgrad).  This file holds the passes the forward never needed:
//   GroupNorm backward : stats (partial sums of q and q * xh per (sample, pixel chunk, group), q = gamma * g) + apply
//                        (dx = res + rstd * (q - m1 - xh * m2)); mean / rstd are re-folded from the FORWARD partials
//                        (the (n, mean, M2, 0) records of az_groupnorm_stats_f32), so nothing but those records is saved
//   row norm backward  : LayerNorm (unbiased variance) / RMSNorm over the channel axis, one wave per pixel row
//   SiLU backward      : y = g * silu'(p) on the PRE-activation p
//   FFN activations    : silu / relu / relu^2 as passes of their own and their pullbacks; the SwiGLU pullback (DiT block)
//   channel scale      : y = x * s[b, c] (the gate c of out = x + c * y, applied to the cotangent)
//   zero stuffing      : the cotangent of a strided convolution on the zero-filled grid of its input
//   nearest upsampling backward : clipped window sums
// Reductions are per-thread sums -> wave butterfly -> LDS in a fixed order: no float atomics, two runs give the same bits.
// A cotangent has no natural range (1e-8 and 1e4 are both ordinary): nothing here assumes O(1) values.
#include "common.h"

namespace {

// Sum of (a, b) over the 256 threads of a block, in a fixed order; every thread gets the result.  `sh`: 8 floats of LDS.
__device__ __forceinline__ void block_sum2(float& a, float& b, float* sh) {
  a = az_wave_sum(a);
  b = az_wave_sum(b);
  const int w = threadIdx.x >> 6;
  __syncthreads();  // (sh may still be read from an earlier call)
  if ((threadIdx.x & 63) == 0) {
    sh[w] = a;
    sh[4 + w] = b;
  }
  __syncthreads();
  a = (sh[0] + sh[1]) + (sh[2] + sh[3]);
  b = (sh[4] + sh[5]) + (sh[6] + sh[7]);
}

// mean and rstd of (sample b, group g) from the forward partials [b][chunk][group] = (n, mean, M2, 0): N = sum n,
// mean = sum(n mean) / N, M2 = sum(M2_i + n_i (mean_i - mean)^2) -- the fold of gn_finalize_kernel (norm.hip), biased variance.
__device__ __forceinline__ void fold_forward(const float* __restrict__ fpart, int fchunks, int groups, int b, int g, float eps,
                                             float* sh, float& mean, float& rstd) {
  const float4* base = reinterpret_cast<const float4*>(fpart) + ((int64_t)b * fchunks * groups + g);
  float N = 0.f, M1 = 0.f;
  for (int i = threadIdx.x; i < fchunks; i += 256) {
    const float4 v = base[(int64_t)i * groups];
    N += v.x;
    M1 += v.x * v.y;
  }
  block_sum2(N, M1, sh);
  mean = M1 / N;
  float M2 = 0.f, unused = 0.f;
  for (int i = threadIdx.x; i < fchunks; i += 256) {
    const float4 v = base[(int64_t)i * groups];
    const float d = v.y - mean;
    M2 += v.z + v.x * d * d;
  }
  block_sum2(M2, unused, sh);
  rstd = rsqrtf(M2 / N + eps);
}

// grid = (nchunks, B, groups).  A block walks the Cg channels of its group over its pixel chunk (float4 where Cg % 4 == 0).
template <bool VEC>
__global__ __launch_bounds__(256) void gn_bwd_stats_kernel(float* __restrict__ bpart, const float* __restrict__ x,
                                                           const float* __restrict__ g, const float* __restrict__ scale,
                                                           int64_t scale_bstride, const float* __restrict__ fpart, int fchunks,
                                                           int64_t HW, int C, int cs, int groups, int nchunks, float eps) {
  __shared__ float sh[8];
  const int chunk = blockIdx.x, b = blockIdx.y, gi = blockIdx.z;
  const int Cg = C / groups;
  float mean, rstd;
  fold_forward(fpart, fchunks, groups, b, gi, eps, sh, mean, rstd);
  const int64_t ppc = (HW + nchunks - 1) / nchunks;
  const int64_t p0 = (int64_t)chunk * ppc;
  const int64_t p1 = p0 + ppc < HW ? p0 + ppc : HW;
  const int64_t np = p1 > p0 ? p1 - p0 : 0;
  const float* sc = scale ? scale + (int64_t)b * scale_bstride : nullptr;
  float s1 = 0.f, s2 = 0.f;
  if (VEC) {
    const int qg = Cg / 4;
    const int64_t total = np * qg;
    for (int64_t e = threadIdx.x; e < total; e += 256) {
      const int64_t p = p0 + e / qg;
      const int c = gi * Cg + 4 * (int)(e % qg);
      const int64_t off = ((int64_t)b * HW + p) * cs + c;
      const float4 xv = *reinterpret_cast<const float4*>(x + off);
      const float4 gv = *reinterpret_cast<const float4*>(g + off);
      const float ga[4] = {sc ? 1.f + sc[c] : 1.f, sc ? 1.f + sc[c + 1] : 1.f, sc ? 1.f + sc[c + 2] : 1.f, sc ? 1.f + sc[c + 3] : 1.f};
      const float xa[4] = {xv.x, xv.y, xv.z, xv.w}, gg[4] = {gv.x, gv.y, gv.z, gv.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float q = ga[j] * gg[j];
        s1 += q;
        s2 += q * ((xa[j] - mean) * rstd);
      }
    }
  } else {
    const int64_t total = np * Cg;
    for (int64_t e = threadIdx.x; e < total; e += 256) {
      const int64_t p = p0 + e / Cg;
      const int c = gi * Cg + (int)(e % Cg);
      const int64_t off = ((int64_t)b * HW + p) * cs + c;
      const float q = (sc ? 1.f + sc[c] : 1.f) * g[off];
      s1 += q;
      s2 += q * ((x[off] - mean) * rstd);
    }
  }
  block_sum2(s1, s2, sh);
  if (threadIdx.x == 0) {
    float* out = bpart + (((int64_t)b * nchunks + chunk) * groups + gi) * 4;
    *reinterpret_cast<float4*>(out) = make_float4(s1, s2, 0.f, 0.f);
  }
}

// grid = (pixel chunks, B, groups [+ 1: the pad lanes]).  dx = res + rstd * (q - m1 - xh * m2).
template <bool VEC>
__global__ __launch_bounds__(256) void gn_bwd_apply_kernel(float* __restrict__ dx, const float* __restrict__ x,
                                                           const float* __restrict__ g, const float* __restrict__ res,
                                                           const float* __restrict__ scale, int64_t scale_bstride,
                                                           const float* __restrict__ fpart, int fchunks,
                                                           const float* __restrict__ bpart, int nchunks, int64_t HW, int C, int cs,
                                                           int groups, float eps) {
  __shared__ float sh[8];
  const int chunk = blockIdx.x, b = blockIdx.y, gi = blockIdx.z;
  const int pchunks = gridDim.x;
  const int64_t ppc = (HW + pchunks - 1) / pchunks;
  const int64_t p0 = (int64_t)chunk * ppc;
  const int64_t p1 = p0 + ppc < HW ? p0 + ppc : HW;
  const int64_t np = p1 > p0 ? p1 - p0 : 0;
  if (gi == groups) {  // pad lanes [C, cs): zero
    const int npad = cs - C;
    for (int64_t e = threadIdx.x; e < np * npad; e += 256)
      dx[((int64_t)b * HW + p0 + e / npad) * cs + C + (int)(e % npad)] = 0.f;
    return;
  }
  const int Cg = C / groups;
  float mean, rstd;
  fold_forward(fpart, fchunks, groups, b, gi, eps, sh, mean, rstd);
  float m1 = 0.f, m2 = 0.f;
  {
    const float4* base = reinterpret_cast<const float4*>(bpart) + ((int64_t)b * nchunks * groups + gi);
    for (int i = threadIdx.x; i < nchunks; i += 256) {
      const float4 v = base[(int64_t)i * groups];
      m1 += v.x;
      m2 += v.y;
    }
    block_sum2(m1, m2, sh);
    const float inv = 1.f / ((float)Cg * (float)HW);
    m1 *= inv;
    m2 *= inv;
  }
  const float* sc = scale ? scale + (int64_t)b * scale_bstride : nullptr;
  if (VEC) {
    const int qg = Cg / 4;
    const int64_t total = np * qg;
    for (int64_t e = threadIdx.x; e < total; e += 256) {
      const int64_t p = p0 + e / qg;
      const int c = gi * Cg + 4 * (int)(e % qg);
      const int64_t off = ((int64_t)b * HW + p) * cs + c;
      const float4 xv = *reinterpret_cast<const float4*>(x + off);
      const float4 gv = *reinterpret_cast<const float4*>(g + off);
      float4 rv = make_float4(0.f, 0.f, 0.f, 0.f);
      if (res) rv = *reinterpret_cast<const float4*>(res + off);
      const float xa[4] = {xv.x, xv.y, xv.z, xv.w}, gg[4] = {gv.x, gv.y, gv.z, gv.w}, ra[4] = {rv.x, rv.y, rv.z, rv.w};
      float o[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float q = (sc ? 1.f + sc[c + j] : 1.f) * gg[j];
        const float xh = (xa[j] - mean) * rstd;
        o[j] = ra[j] + rstd * (q - m1 - xh * m2);
      }
      *reinterpret_cast<float4*>(dx + off) = make_float4(o[0], o[1], o[2], o[3]);
    }
  } else {
    const int64_t total = np * Cg;
    for (int64_t e = threadIdx.x; e < total; e += 256) {
      const int64_t p = p0 + e / Cg;
      const int c = gi * Cg + (int)(e % Cg);
      const int64_t off = ((int64_t)b * HW + p) * cs + c;
      const float q = (sc ? 1.f + sc[c] : 1.f) * g[off];
      const float xh = (x[off] - mean) * rstd;
      dx[off] = (res ? res[off] : 0.f) + rstd * (q - m1 - xh * m2);
    }
  }
}

// One wave per row (pixel).  kind 0: LayerNorm with the UNBIASED variance (xh = (x - mean) rstd, rstd = (var_unb + eps)^-1/2:
// dx = rstd (q - mean(q) - xh mean(q xh) n / (n - 1))); kind 1: RMSNorm (xh = x rstd: dx = rstd (q - xh mean(q xh))).
// HAS_W: a learned per-channel gain under the modulation (y = (1 + scale) weight norm(x) + shift: q = g weight (1 + scale));
// without it the instantiation is the kernel as it was, bit for bit.
template <bool HAS_W>
__global__ __launch_bounds__(256) void rownorm_bwd_kernel(float* __restrict__ dx, const float* __restrict__ x,
                                                          const float* __restrict__ g, const float* __restrict__ res,
                                                          const float* __restrict__ scale, const float* __restrict__ weight,
                                                          int64_t scale_bstride, int64_t rows, int64_t rows_per_batch, int C, int cs,
                                                          int kind, float eps) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t nwaves = (int64_t)gridDim.x * 4;
  for (int64_t row = wave; row < rows; row += nwaves) {
    const float* xr = x + row * cs;
    const float* gr = g + row * cs;
    const float* rr = res ? res + row * cs : nullptr;
    float* yr = dx + row * cs;
    const float* sc = scale ? scale + (row / rows_per_batch) * scale_bstride : nullptr;
    float s = 0.f;
    for (int c = lane; c < C; c += 64) s += kind == 0 ? xr[c] : xr[c] * xr[c];
    s = az_wave_sum(s);
    float mean = 0.f, rstd, corr = 1.f;
    if (kind == 0) {
      mean = s / (float)C;
      float v = 0.f;
      for (int c = lane; c < C; c += 64) {
        const float a = xr[c] - mean;
        v += a * a;
      }
      v = az_wave_sum(v);
      rstd = rsqrtf(v / (float)(C - 1) + eps);
      corr = (float)C / (float)(C - 1);
    } else {
      rstd = rsqrtf(s / (float)C + eps);
    }
    float m1 = 0.f, m2 = 0.f;
    for (int c = lane; c < C; c += 64) {
      const float q = (sc ? 1.f + sc[c] : 1.f) * (HAS_W ? gr[c] * weight[c] : gr[c]);
      m1 += q;
      m2 += q * ((xr[c] - mean) * rstd);
    }
    m1 = kind == 0 ? az_wave_sum(m1) / (float)C : 0.f;
    m2 = az_wave_sum(m2) / (float)C * corr;
    for (int c = lane; c < cs; c += 64) {
      float o = 0.f;
      if (c < C) {
        const float q = (sc ? 1.f + sc[c] : 1.f) * (HAS_W ? gr[c] * weight[c] : gr[c]);
        const float xh = (xr[c] - mean) * rstd;
        o = (rr ? rr[c] : 0.f) + rstd * (q - m1 - xh * m2);
      }
      yr[c] = o;
    }
  }
}

// silu'(p) = s (1 + p (1 - s)), s = 1 / (1 + exp(-p)).  Limits: p -> -inf: s = 0 (1 + exp2(+big) = inf, rcp = 0) and p (1 - s)
// stays finite times 0 = 0 for finite p; p -> +inf: s = 1, p * 0 = 0 for finite p.
__device__ __forceinline__ float silu_grad(float p) {
  const float s = __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(p * -1.4426950408889634f));
  return s * (1.0f + p * (1.0f - s));
}

__global__ __launch_bounds__(256) void silu_bwd_kernel(float* __restrict__ y, const float* __restrict__ g,
                                                       const float* __restrict__ p, int64_t n4) {
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
    const float4 gv = reinterpret_cast<const float4*>(g)[i];
    const float4 pv = reinterpret_cast<const float4*>(p)[i];
    reinterpret_cast<float4*>(y)[i] =
        make_float4(gv.x * silu_grad(pv.x), gv.y * silu_grad(pv.y), gv.z * silu_grad(pv.z), gv.w * silu_grad(pv.w));
  }
}

// FFN activations of the DiT block as passes of their own and their derivatives on the pre-activation p.  kind 1: silu,
// 2: relu, 3: relu(p)^2.
__device__ __forceinline__ float act_val(float p, int kind) {
  if (kind == 1) return az_silu(p);
  const float r = fmaxf(p, 0.f);
  return kind == 2 ? r : r * r;
}
__device__ __forceinline__ float act_grad(float p, int kind) {
  if (kind == 1) return silu_grad(p);
  if (kind == 2) return p > 0.f ? 1.f : 0.f;
  return 2.f * fmaxf(p, 0.f);
}

__global__ __launch_bounds__(256) void act_kernel(float* __restrict__ y, const float* __restrict__ x, int64_t n4, int kind) {
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
    const float4 v = reinterpret_cast<const float4*>(x)[i];
    reinterpret_cast<float4*>(y)[i] = make_float4(act_val(v.x, kind), act_val(v.y, kind), act_val(v.z, kind), act_val(v.w, kind));
  }
}

__global__ __launch_bounds__(256) void act_bwd_kernel(float* __restrict__ y, const float* __restrict__ g, const float* __restrict__ p,
                                                      int64_t n4, int kind) {
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
    const float4 gv = reinterpret_cast<const float4*>(g)[i];
    const float4 pv = reinterpret_cast<const float4*>(p)[i];
    reinterpret_cast<float4*>(y)[i] = make_float4(gv.x * act_grad(pv.x, kind), gv.y * act_grad(pv.y, kind),
                                                  gv.z * act_grad(pv.z, kind), gv.w * act_grad(pv.w, kind));
  }
}

// One thread per two input pairs (a float4 of x): dx[2c] = g silu(x[2c+1]), dx[2c+1] = g x[2c] silu'(x[2c+1]); lanes past 2 cout zero.
__global__ __launch_bounds__(256) void swiglu_bwd_kernel(float* __restrict__ dx, const float* __restrict__ g,
                                                         const float* __restrict__ x, int64_t rows, int cout, int64_t xs, int64_t gs) {
  const int q = (int)(xs / 4);
  const int64_t total = rows * q;
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += stride) {
    const int64_t r = i / q;
    const int c = 2 * (int)(i % q);
    const float4 v = *reinterpret_cast<const float4*>(x + r * xs + 2 * c);
    const float g0 = c < cout ? g[r * gs + c] : 0.f;
    const float g1 = c + 1 < cout ? g[r * gs + c + 1] : 0.f;
    float4 o;
    o.x = c < cout ? g0 * az_silu(v.y) : 0.f;
    o.y = c < cout ? g0 * v.x * silu_grad(v.y) : 0.f;
    o.z = c + 1 < cout ? g1 * az_silu(v.w) : 0.f;
    o.w = c + 1 < cout ? g1 * v.z * silu_grad(v.w) : 0.f;
    *reinterpret_cast<float4*>(dx + r * xs + 2 * c) = o;
  }
}

// y[b, p, c] = x[b, p, c] * s[b * bstride + c]; grid.y = sample.
__global__ __launch_bounds__(256) void channel_scale_kernel(float* __restrict__ y, const float* __restrict__ x,
                                                            const float* __restrict__ s, int64_t bstride, int64_t HW, int C, int cs) {
  const int b = blockIdx.y;
  const int q = cs / 4;
  const int64_t total = HW * q;
  const int64_t stride = (int64_t)gridDim.x * 256;
  const float* sb = s + (int64_t)b * bstride;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += stride) {
    const int c = 4 * (int)(i % q);
    const int64_t off = (int64_t)b * HW * cs + i * 4;
    const float4 v = *reinterpret_cast<const float4*>(x + off);
    float4 o;
    o.x = c < C ? v.x * sb[c] : 0.f;
    o.y = c + 1 < C ? v.y * sb[c + 1] : 0.f;
    o.z = c + 2 < C ? v.z * sb[c + 2] : 0.f;
    o.w = c + 3 < C ? v.w * sb[c + 3] : 0.f;
    *reinterpret_cast<float4*>(y + off) = o;
  }
}

// G[b, Y, X, :] = g[b, Y / sh, X / sw, :] where sh | Y, sw | X and the quotient lies inside g; zero elsewhere.
__global__ __launch_bounds__(256) void zero_stuff_kernel(float* __restrict__ G, const float* __restrict__ g, int64_t B, int h, int w,
                                                         int cs, int sh, int sw, int H, int W) {
  const int q = cs / 4;
  const int64_t total = B * H * W * q;
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += stride) {
    const int c4 = (int)(i % q);
    int64_t p = i / q;
    const int X = (int)(p % W);
    p /= W;
    const int Y = (int)(p % H);
    const int64_t b = p / H;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (Y % sh == 0 && X % sw == 0 && Y / sh < h && X / sw < w)
      v = *reinterpret_cast<const float4*>(g + ((b * h + Y / sh) * w + X / sw) * cs + c4 * 4);
    reinterpret_cast<float4*>(G)[i] = v;
  }
}

// dx[b, i, j, :] = sum of g[b, i sh + di, j sw + dj, :] over di < sh, dj < sw inside the (hn, wn) narrowed map.
__global__ __launch_bounds__(256) void upsample_nearest_bwd_kernel(float* __restrict__ dx, const float* __restrict__ g, int64_t B,
                                                                   int h, int w, int cs, int sh, int sw, int hn, int wn) {
  const int q = cs / 4;
  const int64_t total = B * h * w * q;
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += stride) {
    const int c4 = (int)(i % q);
    int64_t p = i / q;
    const int xj = (int)(p % w);
    p /= w;
    const int yi = (int)(p % h);
    const int64_t b = p / h;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int di = 0; di < sh; ++di) {
      const int Y = yi * sh + di;
      if (Y >= hn) break;
      for (int dj = 0; dj < sw; ++dj) {
        const int X = xj * sw + dj;
        if (X >= wn) break;
        const float4 v = *reinterpret_cast<const float4*>(g + ((b * hn + Y) * wn + X) * cs + c4 * 4);
        acc.x += v.x;
        acc.y += v.y;
        acc.z += v.z;
        acc.w += v.w;
      }
    }
    reinterpret_cast<float4*>(dx)[i] = acc;
  }
}

// The cotangent of the guided mean m = (1 + g) m+ - g m- on the stacked 2B batch: v2 = [(1 + g) v ; -g v].  The second half
// starts at v2 + n, which is 16-byte aligned only when n % 4 == 0: float4 stores where it is, scalar stores otherwise; the
// n % 4 tail is scalar.  12 B / element.
__global__ __launch_bounds__(256) void cfg_split_kernel(float* __restrict__ v2, const float* __restrict__ v,
                                                        const float* __restrict__ g, int64_t n) {
  const float gv = g[0], a = 1.0f + gv, b = -gv;
  const int64_t n4 = n / 4;
  const bool hi4 = n % 4 == 0;
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
    const float4 x = reinterpret_cast<const float4*>(v)[i];
    reinterpret_cast<float4*>(v2)[i] = make_float4(a * x.x, a * x.y, a * x.z, a * x.w);
    float* hi = v2 + n + 4 * i;
    if (hi4) {
      *reinterpret_cast<float4*>(hi) = make_float4(b * x.x, b * x.y, b * x.z, b * x.w);
    } else {
      hi[0] = b * x.x, hi[1] = b * x.y, hi[2] = b * x.z, hi[3] = b * x.w;
    }
  }
  for (int64_t i = 4 * n4 + (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
    const float x = v[i];
    v2[i] = a * x;
    v2[n + i] = b * x;
  }
}

}  // namespace

extern "C" {

int az_groupnorm_bwd_stats_f32(float* bpart, const float* x, const float* g, const float* scale, int64_t scale_bstride,
                               const float* fpart, int32_t fchunks, int64_t B, int64_t HW, int64_t C, int64_t cs, int32_t groups,
                               int32_t nchunks, float eps, az_stream_t stream) {
  AZ_REQUIRE(bpart && x && g && fpart, AZ_E_NULL);
  AZ_REQUIRE(B > 0 && B < 65536 && HW > 0 && C > 0 && cs >= C && cs % 4 == 0 && groups > 0 && groups < 65535 && C % groups == 0 &&
                 nchunks > 0 && fchunks > 0 && scale_bstride >= 0,
             AZ_E_SHAPE);
  AZ_REQUIRE(AZ_ALIGNED16(bpart) && AZ_ALIGNED16(x) && AZ_ALIGNED16(g) && AZ_ALIGNED16(fpart), AZ_E_ALIGN);
  const dim3 grid((unsigned)nchunks, (unsigned)B, (unsigned)groups);
  if ((C / groups) % 4 == 0)
    hipLaunchKernelGGL(gn_bwd_stats_kernel<true>, grid, dim3(256), 0, az_s(stream), bpart, x, g, scale, scale_bstride, fpart,
                       (int)fchunks, HW, (int)C, (int)cs, (int)groups, (int)nchunks, eps);
  else
    hipLaunchKernelGGL(gn_bwd_stats_kernel<false>, grid, dim3(256), 0, az_s(stream), bpart, x, g, scale, scale_bstride, fpart,
                       (int)fchunks, HW, (int)C, (int)cs, (int)groups, (int)nchunks, eps);
  return az_launch_status();
}

int az_groupnorm_bwd_apply_f32(float* dx, const float* x, const float* g, const float* res, const float* scale,
                               int64_t scale_bstride, const float* fpart, int32_t fchunks, const float* bpart, int32_t nchunks,
                               int64_t B, int64_t HW, int64_t C, int64_t cs, int32_t groups, float eps, az_stream_t stream) {
  AZ_REQUIRE(dx && x && g && fpart && bpart, AZ_E_NULL);
  AZ_REQUIRE(B > 0 && B < 65536 && HW > 0 && C > 0 && cs >= C && cs % 4 == 0 && groups > 0 && groups < 65535 && C % groups == 0 &&
                 nchunks > 0 && fchunks > 0 && scale_bstride >= 0,
             AZ_E_SHAPE);
  AZ_REQUIRE(AZ_ALIGNED16(dx) && AZ_ALIGNED16(x) && AZ_ALIGNED16(g) && AZ_ALIGNED16(res) && AZ_ALIGNED16(fpart) && AZ_ALIGNED16(bpart),
             AZ_E_ALIGN);
  const dim3 grid((unsigned)nchunks, (unsigned)B, (unsigned)groups + (cs > C ? 1u : 0u));
  if ((C / groups) % 4 == 0)
    hipLaunchKernelGGL(gn_bwd_apply_kernel<true>, grid, dim3(256), 0, az_s(stream), dx, x, g, res, scale, scale_bstride, fpart,
                       (int)fchunks, bpart, (int)nchunks, HW, (int)C, (int)cs, (int)groups, eps);
  else
    hipLaunchKernelGGL(gn_bwd_apply_kernel<false>, grid, dim3(256), 0, az_s(stream), dx, x, g, res, scale, scale_bstride, fpart,
                       (int)fchunks, bpart, (int)nchunks, HW, (int)C, (int)cs, (int)groups, eps);
  return az_launch_status();
}

int az_rownorm_bwd_f32(float* dx, const float* x, const float* g, const float* res, const float* scale, int64_t scale_bstride,
                       int64_t rows, int64_t rows_per_batch, int64_t C, int64_t cs, int32_t kind, float eps, az_stream_t stream) {
  return az_rownorm_bwd_w_f32(dx, x, g, res, scale, scale_bstride, nullptr, rows, rows_per_batch, C, cs, kind, eps, stream);
}

int az_rownorm_bwd_w_f32(float* dx, const float* x, const float* g, const float* res, const float* scale, int64_t scale_bstride,
                         const float* weight, int64_t rows, int64_t rows_per_batch, int64_t C, int64_t cs, int32_t kind, float eps,
                         az_stream_t stream) {
  AZ_REQUIRE(dx && x && g, AZ_E_NULL);
  AZ_REQUIRE(rows > 0 && rows_per_batch > 0 && C > 0 && cs >= C && cs % 4 == 0 && (kind == 0 || kind == 1) && scale_bstride >= 0 &&
                 (kind == 1 || C > 1),
             AZ_E_SHAPE);
  AZ_REQUIRE(AZ_ALIGNED16(dx) && AZ_ALIGNED16(x) && AZ_ALIGNED16(g) && AZ_ALIGNED16(res), AZ_E_ALIGN);
  int64_t blocks = (rows + 3) / 4;
  if (blocks > 4096) blocks = 4096;
  if (weight != nullptr)
    hipLaunchKernelGGL(rownorm_bwd_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, az_s(stream), dx, x, g, res, scale, weight,
                       scale_bstride, rows, rows_per_batch, (int)C, (int)cs, (int)kind, eps);
  else
    hipLaunchKernelGGL(rownorm_bwd_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, az_s(stream), dx, x, g, res, scale, weight,
                       scale_bstride, rows, rows_per_batch, (int)C, (int)cs, (int)kind, eps);
  return az_launch_status();
}

int az_cfg_split_f32(float* v2, const float* v, const float* g, int64_t n, az_stream_t stream) {
  AZ_REQUIRE(v2 && v && g, AZ_E_NULL);
  AZ_REQUIRE(n > 0, AZ_E_SHAPE);
  AZ_REQUIRE(AZ_ALIGNED16(v2) && AZ_ALIGNED16(v), AZ_E_ALIGN);
  hipLaunchKernelGGL(cfg_split_kernel, dim3(az_stream_grid((n + 3) / 4, 256)), dim3(256), 0, az_s(stream), v2, v, g, n);
  return az_launch_status();
}

int az_silu_bwd_f32(float* y, const float* g, const float* p, int64_t n, az_stream_t stream) {
  AZ_REQUIRE(y && g && p, AZ_E_NULL);
  AZ_REQUIRE(n > 0 && n % 4 == 0, AZ_E_SHAPE);
  AZ_REQUIRE(AZ_ALIGNED16(y) && AZ_ALIGNED16(g) && AZ_ALIGNED16(p), AZ_E_ALIGN);
  hipLaunchKernelGGL(silu_bwd_kernel, dim3(az_stream_grid(n / 4, 256)), dim3(256), 0, az_s(stream), y, g, p, n / 4);
  return az_launch_status();
}

int az_act_f32(float* y, const float* x, int64_t n, int32_t kind, az_stream_t stream) {
  AZ_REQUIRE(y && x, AZ_E_NULL);
  AZ_REQUIRE(n > 0 && n % 4 == 0 && kind >= 1 && kind <= 3, AZ_E_SHAPE);
  AZ_REQUIRE(AZ_ALIGNED16(y) && AZ_ALIGNED16(x), AZ_E_ALIGN);
  hipLaunchKernelGGL(act_kernel, dim3(az_stream_grid(n / 4, 256)), dim3(256), 0, az_s(stream), y, x, n / 4, (int)kind);
  return az_launch_status();
}

int az_act_bwd_f32(float* y, const float* g, const float* p, int64_t n, int32_t kind, az_stream_t stream) {
  AZ_REQUIRE(y && g && p, AZ_E_NULL);
  AZ_REQUIRE(n > 0 && n % 4 == 0 && kind >= 1 && kind <= 3, AZ_E_SHAPE);
  AZ_REQUIRE(AZ_ALIGNED16(y) && AZ_ALIGNED16(g) && AZ_ALIGNED16(p), AZ_E_ALIGN);
  hipLaunchKernelGGL(act_bwd_kernel, dim3(az_stream_grid(n / 4, 256)), dim3(256), 0, az_s(stream), y, g, p, n / 4, (int)kind);
  return az_launch_status();
}

int az_swiglu_bwd_f32(float* dx, const float* g, const float* x, int64_t rows, int64_t cout, int64_t xs, int64_t gs,
                      az_stream_t stream) {
  AZ_REQUIRE(dx && g && x, AZ_E_NULL);
  AZ_REQUIRE(rows > 0 && cout > 0 && cout < (1ll << 30) && xs >= 2 * cout && gs >= cout && xs % 4 == 0, AZ_E_SHAPE);
  AZ_REQUIRE(AZ_ALIGNED16(dx) && AZ_ALIGNED16(x), AZ_E_ALIGN);
  hipLaunchKernelGGL(swiglu_bwd_kernel, dim3(az_stream_grid(rows * (xs / 4), 256)), dim3(256), 0, az_s(stream), dx, g, x, rows,
                     (int)cout, xs, gs);
  return az_launch_status();
}

int az_channel_scale_f32(float* y, const float* x, const float* s, int64_t s_bstride, int64_t B, int64_t HW, int64_t C, int64_t cs,
                         az_stream_t stream) {
  AZ_REQUIRE(y && x && s, AZ_E_NULL);
  AZ_REQUIRE(B > 0 && B < 65536 && HW > 0 && C > 0 && cs >= C && cs % 4 == 0 && s_bstride >= 0, AZ_E_SHAPE);
  AZ_REQUIRE(AZ_ALIGNED16(y) && AZ_ALIGNED16(x), AZ_E_ALIGN);
  int gx = az_stream_grid(HW * (cs / 4), 256);
  const int cap = (int)((2048 + B - 1) / B);
  if (gx > cap) gx = cap;
  hipLaunchKernelGGL(channel_scale_kernel, dim3((unsigned)gx, (unsigned)B), dim3(256), 0, az_s(stream), y, x, s, s_bstride, HW, (int)C,
                     (int)cs);
  return az_launch_status();
}

int az_zero_stuff_f32(float* G, const float* g, int64_t B, int64_t h, int64_t w, int64_t cs, int32_t sh, int32_t sw, int64_t H,
                      int64_t W, az_stream_t stream) {
  AZ_REQUIRE(G && g, AZ_E_NULL);
  AZ_REQUIRE(B > 0 && h > 0 && w > 0 && H > 0 && W > 0 && cs > 0 && cs % 4 == 0 && sh > 0 && sw > 0 && H < (1ll << 31) && W < (1ll << 31),
             AZ_E_SHAPE);
  AZ_REQUIRE((h - 1) * sh <= H - 1 && (w - 1) * sw <= W - 1, AZ_E_SHAPE);  // every element of g lands inside G
  AZ_REQUIRE(AZ_ALIGNED16(G) && AZ_ALIGNED16(g), AZ_E_ALIGN);
  hipLaunchKernelGGL(zero_stuff_kernel, dim3(az_stream_grid(B * H * W * (cs / 4), 256)), dim3(256), 0, az_s(stream), G, g, B, (int)h,
                     (int)w, (int)cs, (int)sh, (int)sw, (int)H, (int)W);
  return az_launch_status();
}

int az_upsample_nearest_bwd_f32(float* dx, const float* g, int64_t B, int64_t h, int64_t w, int64_t cs, int32_t sh, int32_t sw,
                                int64_t hn, int64_t wn, az_stream_t stream) {
  AZ_REQUIRE(dx && g, AZ_E_NULL);
  AZ_REQUIRE(B > 0 && h > 0 && w > 0 && hn > 0 && wn > 0 && cs > 0 && cs % 4 == 0 && sh > 0 && sw > 0 && h < (1ll << 31) &&
                 w < (1ll << 31),
             AZ_E_SHAPE);
  AZ_REQUIRE(hn <= h * sh && wn <= w * sw, AZ_E_SHAPE);  // the narrowed map lies inside the upsampled one
  AZ_REQUIRE(AZ_ALIGNED16(dx) && AZ_ALIGNED16(g), AZ_E_ALIGN);
  hipLaunchKernelGGL(upsample_nearest_bwd_kernel, dim3(az_stream_grid(B * h * w * (cs / 4), 256)), dim3(256), 0, az_s(stream), dx, g,
                     B, (int)h, (int)w, (int)cs, (int)sh, (int)sw, (int)hn, (int)wn);
  return az_launch_status();
}

}  // extern "C"
