// Input-gradient kernels of the ADM (guided-diffusion) UNet on the channel-padded NHWC layout.  All fp32, all HBM-bound.
//
//   norm-affine pullback : the ADM norm pass y = pool(act(S[b,c] x + T[b,c])) (az_groupnorm_finalize_f32 + az_affine_act_f32:
//                          GroupNorm, its affine, FiLM, SiLU and the average pool in one pass) on the way back.  With
//                          S = r_g m_c, m_c = gamma_c (1 + scale[b,c]), r_g the group's reciprocal standard deviation and
//                          xh = (x - mean_g) r_g:
//                              u  = pool^T(g) act'(S x + T)          (act' RECOMPUTED from x: no pre-activation is kept)
//                              s1 = sum_group m u,  s2 = sum_group m u xh
//                              dx = r_g (m u - s1 / N - xh s2 / N) [+ res]
//                          stats (partial (s1, s2) per (sample, pixel chunk, group)) + apply.  The input may be the channel
//                          concatenation x0 | x1 read in place (groups may straddle the boundary); dx goes to one tensor per
//                          source.  mean_g / r_g are re-folded from the FORWARD partials ((n, mean, M2, 0) records of
//                          az_groupnorm_stats_f32), never from E[x^2] - E[x]^2.
//   average-pool pullback: dx = pool^T(g) [+ res] of the pooling-only pass
//   ADM preconditioning  : mean = clip(c_skip x_t + c_out eps) on the way back, in two elementwise passes
// Reductions: per-thread sums -> LDS -> one leader per group in a fixed order; partials of the pixel chunks are folded by one
// wave per group (butterfly).  No float atomics: two runs give the same bits.  Cotangents have no natural range.
#include "common.h"

namespace {

// silu'(p) = s (1 + p (1 - s)), s = 1 / (1 + exp(-p)) (as backward.hip)
__device__ __forceinline__ float silu_grad(float p) {
  const float s = __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(p * -1.4426950408889634f));
  return s * (1.0f + p * (1.0f - s));
}

struct NormBwd {
  const float* x0;     // source 0: (B, HW, c0s) when x1 is given, else (B, HW, cs)
  const float* x1;     // source 1: (B, HW, cs - c0s), or null
  const float* g;      // cotangent of y on the (pooled) output grid, (B, HWo, cs)
  const float* S;      // (B, cs)
  const float* T;      // (B, cs)
  const float* weight; // gamma (C) or null
  const float* scale;  // FiLM scale (b * scale_bstride + c) or null
  const float* fpart;  // forward partials [b][fchunk][group] (n, mean, M2, 0)
  float* bpart;        // backward partials [b][chunk][group] (s1, s2, 0, 0)
  float* dx0;
  float* dx1;
  const float* res0;
  const float* res1;
  int64_t scale_bstride;
  int c0s, C, cs, groups, H, W, act, pool, fchunks, nchunks;
  float eps;
};

// mean / rstd of group g of sample b by ONE wave (lanes over the forward partials; the fold of gn_finalize_kernel, norm.hip)
__device__ __forceinline__ void wave_fold_forward(const NormBwd& a, int b, int g, int lane, float& mean, float& rstd) {
  const float4* base = reinterpret_cast<const float4*>(a.fpart) + ((int64_t)b * a.fchunks * a.groups + g);
  float N = 0.f, M1 = 0.f;
  for (int i = lane; i < a.fchunks; i += 64) {
    const float4 v = base[(int64_t)i * a.groups];
    N += v.x;
    M1 += v.x * v.y;
  }
  N = az_wave_sum(N);
  M1 = az_wave_sum(M1);
  mean = M1 / N;
  float M2 = 0.f;
  for (int i = lane; i < a.fchunks; i += 64) {
    const float4 v = base[(int64_t)i * a.groups];
    const float d = v.y - mean;
    M2 += v.z + v.x * d * d;
  }
  M2 = az_wave_sum(M2);
  rstd = rsqrtf(M2 / N + a.eps);
}

// (s1, s2) / N of group g of sample b by one wave (lanes over the backward partials of the pixel chunks)
__device__ __forceinline__ void wave_fold_backward(const NormBwd& a, int b, int g, int lane, float& m1, float& m2) {
  const float4* base = reinterpret_cast<const float4*>(a.bpart) + ((int64_t)b * a.nchunks * a.groups + g);
  float s1 = 0.f, s2 = 0.f;
  for (int i = lane; i < a.nchunks; i += 64) {
    const float4 v = base[(int64_t)i * a.groups];
    s1 += v.x;
    s2 += v.y;
  }
  const float inv = 1.f / ((float)(a.C / a.groups) * (float)a.H * (float)a.W);
  m1 = az_wave_sum(s1) * inv;
  m2 = az_wave_sum(s2) * inv;
}

// index of the output pixel whose pooling window holds input pixel p, and the window's weight
__device__ __forceinline__ int pooled_pixel(int p, int W, int pool) {
  if (pool == 0) return p;
  const int h = p / W, w = p - h * W;
  return (pool == 1 ? (h >> 1) : h) * (W >> 1) + (w >> 1);
}

// m_c = gamma_c (1 + scale[b, c])
__device__ __forceinline__ float mod_gain(const NormBwd& a, int b, int c) {
  const float w = a.weight ? a.weight[c] : 1.f;
  return a.scale ? w * (1.f + a.scale[(int64_t)b * a.scale_bstride + c]) : w;
}

// u = pool^T(g) act'(S x + T)
__device__ __forceinline__ float cot(float g, float x, float S, float T, float pw, int act) {
  const float u = g * pw;
  return act == 1 ? u * silu_grad(fmaf(x, S, T)) : u;
}

// Fast path: whole 4-channel quads per group (Cg % 4 == 0).  A block owns a slice of `qs` <= 64 quads holding whole groups
// (at most 64 of them) over one pixel chunk: thread -> (quad tid % qs, pixel lane tid / qs), so a wave reads contiguous rows.
// grid = (nchunks, B, slices [+ 1 in APPLY: the pad lanes]).
template <bool APPLY>
__global__ __launch_bounds__(256) void norm_affine_bwd_vec_kernel(NormBwd a, int qs) {
  __shared__ float sh_a[256], sh_b[256];
  __shared__ float sh_mean[64], sh_rstd[64], sh_m1[64], sh_m2[64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int chunk = blockIdx.x, b = blockIdx.y, z = blockIdx.z;
  const int HW = a.H * a.W;
  const int ppc = (HW + a.nchunks - 1) / a.nchunks;
  const int p0 = chunk * ppc;
  const int p1 = p0 + ppc < HW ? p0 + ppc : HW;
  if (APPLY && z * qs * 4 >= a.C) {  // pad lanes [C, cs) of a one-source tensor: zero
    const int npad = a.cs - a.C;
    const int np = p1 > p0 ? p1 - p0 : 0;
    for (int e = tid; e < np * npad; e += 256)
      a.dx0[((int64_t)b * HW + p0 + e / npad) * a.cs + a.C + e % npad] = 0.f;
    return;
  }
  const int Cg = a.C / a.groups;
  const int qg = Cg / 4;         // quads per group
  const int ngs = qs / qg;       // groups of this slice
  const int g_lo = (z * qs) / qg;
  for (int gl = wave; gl < ngs; gl += 4) {
    float mean, rstd;
    wave_fold_forward(a, b, g_lo + gl, lane, mean, rstd);
    float m1 = 0.f, m2 = 0.f;
    if (APPLY) wave_fold_backward(a, b, g_lo + gl, lane, m1, m2);
    if (lane == 0) {
      sh_mean[gl] = mean;
      sh_rstd[gl] = rstd;
      sh_m1[gl] = m1;
      sh_m2[gl] = m2;
    }
  }
  __syncthreads();
  const int ql = tid % qs, pl = tid / qs, ppi = 256 / qs;
  const int c = (z * qs + ql) * 4;
  const bool live = pl < ppi;
  float s1 = 0.f, s2 = 0.f;
  if (live) {
    const int gl = ql / qg;
    const float mean = sh_mean[gl], rstd = sh_rstd[gl];
    const float m1 = sh_m1[gl], m2 = sh_m2[gl];
    const bool second = a.x1 != nullptr && c >= a.c0s;
    const int scs = a.x1 == nullptr ? a.cs : (second ? a.cs - a.c0s : a.c0s);
    const int sc_ = second ? c - a.c0s : c;
    const float* src = second ? a.x1 : a.x0;
    const float* res = second ? a.res1 : a.res0;
    float* dst = second ? a.dx1 : a.dx0;
    const float4 Sv = *reinterpret_cast<const float4*>(a.S + (int64_t)b * a.cs + c);
    const float4 Tv = *reinterpret_cast<const float4*>(a.T + (int64_t)b * a.cs + c);
    const float Sa[4] = {Sv.x, Sv.y, Sv.z, Sv.w}, Ta[4] = {Tv.x, Tv.y, Tv.z, Tv.w};
    float ma[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) ma[j] = mod_gain(a, b, c + j);
    const float pw = a.pool == 0 ? 1.f : (a.pool == 1 ? 0.25f : 0.5f);
    const int HWo = a.pool == 0 ? HW : (a.pool == 1 ? HW / 4 : HW / 2);
    for (int p = p0 + pl; p < p1; p += ppi) {
      const int64_t off = ((int64_t)b * HW + p) * scs + sc_;
      const float4 xv = *reinterpret_cast<const float4*>(src + off);
      const float4 gv = *reinterpret_cast<const float4*>(a.g + ((int64_t)b * HWo + pooled_pixel(p, a.W, a.pool)) * a.cs + c);
      const float xa[4] = {xv.x, xv.y, xv.z, xv.w}, ga[4] = {gv.x, gv.y, gv.z, gv.w};
      if (!APPLY) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float q = ma[j] * cot(ga[j], xa[j], Sa[j], Ta[j], pw, a.act);
          s1 += q;
          s2 += q * ((xa[j] - mean) * rstd);
        }
      } else {
        float4 rv = make_float4(0.f, 0.f, 0.f, 0.f);
        if (res) rv = *reinterpret_cast<const float4*>(res + off);
        const float ra[4] = {rv.x, rv.y, rv.z, rv.w};
        float o[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float q = ma[j] * cot(ga[j], xa[j], Sa[j], Ta[j], pw, a.act);
          const float xh = (xa[j] - mean) * rstd;
          o[j] = ra[j] + rstd * (q - m1 - xh * m2);
        }
        *reinterpret_cast<float4*>(dst + off) = make_float4(o[0], o[1], o[2], o[3]);
      }
    }
  }
  if (APPLY) return;
  sh_a[tid] = s1;
  sh_b[tid] = s2;
  __syncthreads();
  if (tid < ngs) {  // one leader per group: its quads x pixel lanes in a fixed order
    float t1 = 0.f, t2 = 0.f;
    for (int k = 0; k < ppi; ++k)
      for (int j = 0; j < qg; ++j) {
        t1 += sh_a[k * qs + tid * qg + j];
        t2 += sh_b[k * qs + tid * qg + j];
      }
    float* out = a.bpart + (((int64_t)b * a.nchunks + chunk) * a.groups + g_lo + tid) * 4;
    *reinterpret_cast<float4*>(out) = make_float4(t1, t2, 0.f, 0.f);
  }
}

// Generic path (any group size, e.g. 96 channels in 32 groups of 3): grid = (nchunks, B, groups [+ 1: pad lanes]), scalar accesses.
template <bool APPLY>
__global__ __launch_bounds__(256) void norm_affine_bwd_generic_kernel(NormBwd a) {
  __shared__ float sh_a[4], sh_b[4];
  __shared__ float sh_stat[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int chunk = blockIdx.x, b = blockIdx.y, gi = blockIdx.z;
  const int HW = a.H * a.W;
  const int ppc = (HW + a.nchunks - 1) / a.nchunks;
  const int p0 = chunk * ppc;
  const int p1 = p0 + ppc < HW ? p0 + ppc : HW;
  const int np = p1 > p0 ? p1 - p0 : 0;
  if (APPLY && gi == a.groups) {
    const int npad = a.cs - a.C;
    for (int e = tid; e < np * npad; e += 256)
      a.dx0[((int64_t)b * HW + p0 + e / npad) * a.cs + a.C + e % npad] = 0.f;
    return;
  }
  if (wave == 0) {
    float mean, rstd, m1 = 0.f, m2 = 0.f;
    wave_fold_forward(a, b, gi, lane, mean, rstd);
    if (APPLY) wave_fold_backward(a, b, gi, lane, m1, m2);
    if (lane == 0) {
      sh_stat[0] = mean;
      sh_stat[1] = rstd;
      sh_stat[2] = m1;
      sh_stat[3] = m2;
    }
  }
  __syncthreads();
  const float mean = sh_stat[0], rstd = sh_stat[1], m1 = sh_stat[2], m2 = sh_stat[3];
  const int Cg = a.C / a.groups;
  const float pw = a.pool == 0 ? 1.f : (a.pool == 1 ? 0.25f : 0.5f);
  const int HWo = a.pool == 0 ? HW : (a.pool == 1 ? HW / 4 : HW / 2);
  float s1 = 0.f, s2 = 0.f;
  for (int e = tid; e < np * Cg; e += 256) {
    const int p = p0 + e / Cg;
    const int c = gi * Cg + e % Cg;
    const bool second = a.x1 != nullptr && c >= a.c0s;
    const int scs = a.x1 == nullptr ? a.cs : (second ? a.cs - a.c0s : a.c0s);
    const int64_t off = ((int64_t)b * HW + p) * scs + (second ? c - a.c0s : c);
    const float xv = (second ? a.x1 : a.x0)[off];
    const float gv = a.g[((int64_t)b * HWo + pooled_pixel(p, a.W, a.pool)) * a.cs + c];
    const float q = mod_gain(a, b, c) * cot(gv, xv, a.S[(int64_t)b * a.cs + c], a.T[(int64_t)b * a.cs + c], pw, a.act);
    const float xh = (xv - mean) * rstd;
    if (!APPLY) {
      s1 += q;
      s2 += q * xh;
    } else {
      const float* res = second ? a.res1 : a.res0;
      (second ? a.dx1 : a.dx0)[off] = (res ? res[off] : 0.f) + rstd * (q - m1 - xh * m2);
    }
  }
  if (APPLY) return;
  s1 = az_wave_sum(s1);
  s2 = az_wave_sum(s2);
  if (lane == 0) {
    sh_a[wave] = s1;
    sh_b[wave] = s2;
  }
  __syncthreads();
  if (tid == 0) {
    float* out = a.bpart + (((int64_t)b * a.nchunks + chunk) * a.groups + gi) * 4;
    *reinterpret_cast<float4*>(out) = make_float4((sh_a[0] + sh_a[1]) + (sh_a[2] + sh_a[3]), (sh_b[0] + sh_b[1]) + (sh_b[2] + sh_b[3]), 0.f, 0.f);
  }
}

// dx[b, h, w, :] = pw g[b, h / ph, w / 2, :] [+ res]; PH = rows of the pooling window
__global__ __launch_bounds__(256) void avgpool_bwd_kernel(float* __restrict__ dx, const float* __restrict__ g, const float* __restrict__ res,
                                                          int64_t B, int H, int W, int cs, int pool) {
  const int q = cs / 4;
  const int64_t total = B * H * W * q;
  const int64_t stride = (int64_t)gridDim.x * 256;
  const float pw = pool == 1 ? 0.25f : 0.5f;
  const int Ho = pool == 1 ? H / 2 : H, Wo = W / 2;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += stride) {
    const int c4 = (int)(i % q);
    int64_t p = i / q;
    const int w = (int)(p % W);
    p /= W;
    const int h = (int)(p % H);
    const int64_t b = p / H;
    const float4 v = *reinterpret_cast<const float4*>(g + ((b * Ho + (pool == 1 ? h >> 1 : h)) * Wo + (w >> 1)) * cs + c4 * 4);
    float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
    if (res) r = reinterpret_cast<const float4*>(res)[i];
    reinterpret_cast<float4*>(dx)[i] = make_float4(r.x + pw * v.x, r.y + pw * v.y, r.z + pw * v.z, r.w + pw * v.w);
  }
}

// gF[b, f, i] = c_out[b] mask v[b, f, i] for f < C, 0 for C <= f < F; mask = the kept mean lies strictly inside (lo, hi)
// (a clipped element sits exactly ON a bound; without clipping lo / hi are infinite and every finite mean passes).
__global__ __launch_bounds__(256) void adm_precond_bwd_out_kernel(float* __restrict__ gF, const float* __restrict__ v,
                                                                  const float* __restrict__ mean, const float* __restrict__ c_out,
                                                                  int per_sample, int64_t B, int C, int F, int64_t inner, float lo, float hi) {
  const int64_t total = B * F * inner;
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += stride) {
    const int64_t b = i / ((int64_t)F * inner);
    const int64_t r = i - b * F * inner;
    float o = 0.f;
    if (r < (int64_t)C * inner) {
      const int64_t j = b * C * inner + r;
      const float m = mean[j];
      o = (m > lo && m < hi) ? c_out[per_sample ? b : 0] * v[j] : 0.f;
    }
    gF[i] = o;
  }
}

// dx = c_in g + c_skip mask v
__global__ __launch_bounds__(256) void adm_precond_bwd_in_kernel(float* __restrict__ dx, const float* __restrict__ g, const float* __restrict__ v,
                                                                 const float* __restrict__ mean, const float* __restrict__ c_in,
                                                                 const float* __restrict__ c_skip, int per_sample, int64_t B, int64_t n,
                                                                 float lo, float hi) {
  const int64_t total = B * n;
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += stride) {
    const int64_t b = per_sample ? i / n : 0;
    const float m = mean[i];
    const float o = c_in[b] * g[i];
    dx[i] = (m > lo && m < hi) ? fmaf(c_skip[b], v[i], o) : o;
  }
}

int norm_affine_check(const NormBwd& a, int64_t B) {
  AZ_REQUIRE(a.x0 && a.g && a.S && a.T && a.fpart && a.bpart, AZ_E_NULL);
  AZ_REQUIRE(B > 0 && B < 65536 && a.H > 0 && a.W > 0 && (int64_t)a.H * a.W < (1ll << 31) && a.C > 0 && a.cs >= a.C && a.cs % 4 == 0 &&
                 a.groups > 0 && a.groups < 65535 && a.C % a.groups == 0 && a.nchunks > 0 && a.nchunks < 65536 && a.fchunks > 0 &&
                 a.scale_bstride >= 0 && (a.act == 0 || a.act == 1) && a.pool >= 0 && a.pool <= 2,
             AZ_E_SHAPE);
  if (a.x1) AZ_REQUIRE(a.c0s > 0 && a.c0s < a.cs && a.c0s % 4 == 0 && a.C == a.cs, AZ_E_SHAPE);
  if (a.pool == 1) AZ_REQUIRE(a.H % 2 == 0 && a.W % 2 == 0, AZ_E_SHAPE);
  if (a.pool == 2) AZ_REQUIRE(a.W % 2 == 0, AZ_E_SHAPE);
  AZ_REQUIRE(AZ_ALIGNED16(a.x0) && AZ_ALIGNED16(a.x1) && AZ_ALIGNED16(a.g) && AZ_ALIGNED16(a.S) && AZ_ALIGNED16(a.T) &&
                 AZ_ALIGNED16(a.fpart) && AZ_ALIGNED16(a.bpart),
             AZ_E_ALIGN);
  return AZ_OK;
}

// quads per slice of the fast path: the largest divisor of C / 4, at most 64, that holds whole groups (0: the generic kernel)
int slice_quads(int C, int groups) {
  const int Cg = C / groups;
  if (Cg % 4 != 0 || Cg > 256) return 0;
  const int q = C / 4;
  for (int d = q < 64 ? q : 64; d >= Cg / 4; --d)
    if (q % d == 0 && (4 * d) % Cg == 0) return d;
  return 0;
}

template <bool APPLY>
int norm_affine_launch(const NormBwd& a, int64_t B, az_stream_t stream) {
  const int qs = slice_quads(a.C, a.groups);
  const unsigned padz = (APPLY && a.cs > a.C) ? 1u : 0u;
  if (qs > 0) {
    const dim3 grid((unsigned)a.nchunks, (unsigned)B, (unsigned)(a.C / 4 / qs) + padz);
    hipLaunchKernelGGL(norm_affine_bwd_vec_kernel<APPLY>, grid, dim3(256), 0, az_s(stream), a, qs);
  } else {
    const dim3 grid((unsigned)a.nchunks, (unsigned)B, (unsigned)a.groups + padz);
    hipLaunchKernelGGL(norm_affine_bwd_generic_kernel<APPLY>, grid, dim3(256), 0, az_s(stream), a);
  }
  return az_launch_status();
}

}  // namespace

extern "C" {

int az_norm_affine_bwd_stats_f32(float* bpart, const float* x0, const float* x1, int64_t c0s, const float* g, const float* S,
                                 const float* T, const float* weight, const float* scale, int64_t scale_bstride, const float* fpart,
                                 int32_t fchunks, int64_t B, int64_t H, int64_t W, int64_t C, int64_t cs, int32_t groups,
                                 int32_t nchunks, int32_t act, int32_t pool, float eps, az_stream_t stream) {
  AZ_REQUIRE(H < (1ll << 31) && W < (1ll << 31) && C < (1ll << 31) && cs < (1ll << 31) && c0s >= 0 && c0s < (1ll << 31), AZ_E_SHAPE);
  NormBwd a = {};
  a.x0 = x0, a.x1 = x1, a.g = g, a.S = S, a.T = T, a.weight = weight, a.scale = scale, a.fpart = fpart, a.bpart = bpart;
  a.scale_bstride = scale_bstride;
  a.c0s = (int)c0s, a.C = (int)C, a.cs = (int)cs, a.groups = groups, a.H = (int)H, a.W = (int)W, a.act = act, a.pool = pool;
  a.fchunks = fchunks, a.nchunks = nchunks, a.eps = eps;
  const int rc = norm_affine_check(a, B);
  if (rc != AZ_OK) return rc;
  return norm_affine_launch<false>(a, B, stream);
}

int az_norm_affine_bwd_apply_f32(float* dx0, float* dx1, const float* res0, const float* res1, const float* x0, const float* x1,
                                 int64_t c0s, const float* g, const float* S, const float* T, const float* weight, const float* scale,
                                 int64_t scale_bstride, const float* fpart, int32_t fchunks, const float* bpart, int32_t nchunks,
                                 int64_t B, int64_t H, int64_t W, int64_t C, int64_t cs, int32_t groups, int32_t act, int32_t pool,
                                 float eps, az_stream_t stream) {
  AZ_REQUIRE(H < (1ll << 31) && W < (1ll << 31) && C < (1ll << 31) && cs < (1ll << 31) && c0s >= 0 && c0s < (1ll << 31), AZ_E_SHAPE);
  NormBwd a = {};
  a.x0 = x0, a.x1 = x1, a.g = g, a.S = S, a.T = T, a.weight = weight, a.scale = scale, a.fpart = fpart;
  a.bpart = const_cast<float*>(bpart);
  a.dx0 = dx0, a.dx1 = dx1, a.res0 = res0, a.res1 = res1;
  a.scale_bstride = scale_bstride;
  a.c0s = (int)c0s, a.C = (int)C, a.cs = (int)cs, a.groups = groups, a.H = (int)H, a.W = (int)W, a.act = act, a.pool = pool;
  a.fchunks = fchunks, a.nchunks = nchunks, a.eps = eps;
  AZ_REQUIRE(dx0 && (x1 == nullptr || dx1), AZ_E_NULL);
  const int rc = norm_affine_check(a, B);
  if (rc != AZ_OK) return rc;
  AZ_REQUIRE(AZ_ALIGNED16(dx0) && AZ_ALIGNED16(dx1) && AZ_ALIGNED16(res0) && AZ_ALIGNED16(res1), AZ_E_ALIGN);
  return norm_affine_launch<true>(a, B, stream);
}

int az_avgpool_bwd_f32(float* dx, const float* g, const float* res, int64_t B, int64_t H, int64_t W, int64_t cs, int32_t pool,
                       az_stream_t stream) {
  AZ_REQUIRE(dx && g, AZ_E_NULL);
  AZ_REQUIRE(B > 0 && H > 0 && W > 0 && H < (1ll << 31) && W < (1ll << 31) && cs > 0 && cs < (1ll << 31) && cs % 4 == 0 &&
                 (pool == 1 || pool == 2) && W % 2 == 0 && (pool == 2 || H % 2 == 0),
             AZ_E_SHAPE);
  AZ_REQUIRE(AZ_ALIGNED16(dx) && AZ_ALIGNED16(g) && AZ_ALIGNED16(res), AZ_E_ALIGN);
  hipLaunchKernelGGL(avgpool_bwd_kernel, dim3(az_stream_grid(B * H * W * (cs / 4), 256)), dim3(256), 0, az_s(stream), dx, g, res, B,
                     (int)H, (int)W, (int)cs, (int)pool);
  return az_launch_status();
}

int az_adm_precond_bwd_out_f32(float* gF, const float* v, const float* mean, const float* c_out, int32_t per_sample, int64_t B,
                               int64_t C, int64_t F, int64_t inner, float lo, float hi, az_stream_t stream) {
  AZ_REQUIRE(gF && v && mean && c_out, AZ_E_NULL);
  AZ_REQUIRE(B > 0 && C > 0 && F >= C && F < (1ll << 31) && inner > 0 && lo < hi, AZ_E_SHAPE);
  hipLaunchKernelGGL(adm_precond_bwd_out_kernel, dim3(az_stream_grid(B * F * inner, 256)), dim3(256), 0, az_s(stream), gF, v, mean,
                     c_out, (int)(per_sample != 0), B, (int)C, (int)F, inner, lo, hi);
  return az_launch_status();
}

int az_adm_precond_bwd_in_f32(float* dx, const float* g, const float* v, const float* mean, const float* c_in, const float* c_skip,
                              int32_t per_sample, int64_t B, int64_t n, float lo, float hi, az_stream_t stream) {
  AZ_REQUIRE(dx && g && v && mean && c_in && c_skip, AZ_E_NULL);
  AZ_REQUIRE(B > 0 && n > 0 && lo < hi, AZ_E_SHAPE);
  hipLaunchKernelGGL(adm_precond_bwd_in_kernel, dim3(az_stream_grid(B * n, 256)), dim3(256), 0, az_s(stream), dx, g, v, mean, c_in,
                     c_skip, (int)(per_sample != 0), B, n, lo, hi);
  return az_launch_status();
}

}  // extern "C"
