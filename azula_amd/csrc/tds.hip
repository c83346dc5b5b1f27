// Twisted diffusion sampler (azula/guidance/tds.py:70-102): the non-network part of TDSSampler.step as two launches.
//
// az_tds_resample_f32 (tds.py:70-78) -- ONE workgroup of 1024 threads.
//   log_w = log_p (+ log_w_prev), w = softmax(log_w), ancestors[j] = min{ i : c_i > u_j } with c the inclusive prefix sum of w
//   (multinomial sampling with replacement by inverse CDF on the caller's uniforms; not torch.multinomial's stream).
//   Thread t owns the contiguous segment [t * seg, (t + 1) * seg), seg = ceil(K / 1024) <= 64.  log_w, its maximum and
//   e_i = exp(log_w_i - max) are formed in fp64 (log_p + log_w_prev is exact there); e_i is kept as a float in the `w` buffer.
//   The CDF is UN-normalised and fp64: a segment's sum is a sequential fp64 sum, the 1024 segment ends are a sequential fp64 scan
//   by one thread in LDS (base[s + 1] = base[s] + sum_s), and c_i = base[s] + (e_first + ... + e_i).  Both levels only ever
//   add non-negative values to a running sum, so c is monotone, c at a segment's last element IS base[s + 1], and the search
//   for v = u_j * c_{K-1} (binary over base[] in LDS, then a walk of at most 64 elements) always ends on an element with
//   e_i > 0: a particle of weight 0 (log-weight -inf) is never chosen.  w_i = e_i / c_{K-1} is written last.
//   Degenerate input (a NaN, a +inf, or every log-weight -inf -- the reference raises inside torch.multinomial there):
//   w = NaN and ancestors[j] = j.
//
// az_tds_propose_f32 (tds.py:80-102) -- one streaming pass that gathers by ancestor, proposes, samples and reweights, and a
// finishing launch of one thread per particle.  With k = ancestors[j] and the coefficients
// [a_t, a_s, c_s = sigma_t^2 / alpha_t, k_x = sigma_s sqrt(tau) / sigma_t, scale = sigma_s sqrt(1 - tau), 1 / scale]:
//   m      = x_hat[k] + c_s * score[k]
//   x_s[j] = a_s * m + k_x * (x_t[k] - a_t * m) + scale * z[j]                       (4 fused multiply-adds and 1 multiply)
//   log_w_next[j] = -sum_i (z g + g^2 / 2) - log_p[k],   g = (a_s - k_x a_t) c_s score[k] / scale
// The reference forms the weight as log q_s(x_s) - log q_{s|y}(x_s): two fp32 sums of N log-densities whose difference is the
// weight.  Both Normals share their scale and x_s = loc_y + scale z, so the difference of the two quadratics is
// -(z g + g^2 / 2) per element with g = (loc_y - loc) / scale; nothing cancels between large sums.
// Accumulation (fixed order, no atomics; Test B of tests/test_gpu_tds_kernels.py rests on these counts):
//   * a term is evaluated in fp64 (the factor of g is formed once per thread in fp64 from a_t, a_s, c_s, k_x and scale; the
//     1 / scale slot is not read) and rounded ONCE to fp32;
//   * a thread sums the at most 16 terms of one span (4096 elements of a row) in four fp32 accumulators of at most 4 terms
//     and combines them as (a0 + a1) + (a2 + a3): the longest chain of dependent fp32 adds is 3 + 2 = 5;
//   * that fp32 partial is added to the thread's fp64 sum; lanes (butterfly), waves (LDS), the chunks of a row (workspace,
//     summed sequentially by the finishing thread) and log_p[k] are all combined in fp64; the result is rounded once to fp32.
//   So |error| <= (1 + 5 + 1) * 2^-24 * (sum_i |term_i| + |log_p[k]|) to first order; the tests use c = 8.
// Grid: az_tds_chunks(K, N) workgroups per particle, K * chunks <= max(K, 2048) in all; a workgroup strides over the spans of
// its row.  Rows whose length is a multiple of 4 move as 16-byte non-temporal streams; other lengths leave the rows of a
// contiguous (K, N) tensor unaligned, and every access is a 4-byte one (same spans, same accumulation order per thread).
// An ancestor outside [0, K) reads nothing: that particle's x_s and log_w_next are NaN.
#include "common.h"

#include <math.h>

namespace {

constexpr int RS_THREADS = 1024;
constexpr int RS_MAX_K = 65536;

__global__ __launch_bounds__(RS_THREADS) void tds_resample_kernel(const float* __restrict__ log_p,
                                                                  const float* __restrict__ log_w_prev,
                                                                  const float* __restrict__ u, int64_t* __restrict__ anc,
                                                                  float* w, int K) {
  __shared__ double base[RS_THREADS + 1];
  __shared__ double wave_max[RS_THREADS / AZ_WAVE];
  const int tid = threadIdx.x, lane = tid & (AZ_WAVE - 1), wave = tid / AZ_WAVE;
  const int seg = (K + RS_THREADS - 1) / RS_THREADS;
  const int lo = min(K, tid * seg), hi = min(K, lo + seg);
  auto log_w = [&](int i) { return log_w_prev ? (double)log_p[i] + (double)log_w_prev[i] : (double)log_p[i]; };

  double m = -INFINITY;
  int bad = 0;
  for (int i = lo; i < hi; ++i) {
    const double v = log_w(i);
    bad |= (v != v);
    m = fmax(m, v);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmax(m, __shfl_xor(m, o, 64));
  if (lane == 0) wave_max[wave] = m;
  __syncthreads();
  m = wave_max[0];
  for (int i = 1; i < RS_THREADS / AZ_WAVE; ++i) m = fmax(m, wave_max[i]);
  bad |= !(fabs(m) < INFINITY);  // every log-weight -inf, or a +inf
  if (__syncthreads_or(bad)) {
    for (int j = tid; j < K; j += RS_THREADS) {
      w[j] = __builtin_nanf("");
      anc[j] = j;
    }
    return;
  }

  double run = 0.0;
  for (int i = lo; i < hi; ++i) {
    const float e = (float)exp(log_w(i) - m);
    w[i] = e;
    run += (double)e;
  }
  base[tid + 1] = run;
  __syncthreads();
  if (tid == 0) {
    double acc = 0.0;
    base[0] = 0.0;
    for (int s = 0; s < RS_THREADS; ++s) {
      acc += base[s + 1];
      base[s + 1] = acc;
    }
  }
  __syncthreads();  // (also orders the e_i stores above before the walks below)
  const double total = base[RS_THREADS];

  for (int j = tid; j < K; j += RS_THREADS) {
    const double v = (double)u[j] * total;
    int a = 0, b = RS_THREADS - 1;  // s = min{ s : base[s + 1] > v }
    while (a < b) {
      const int mid = (a + b) >> 1;
      if (base[mid + 1] > v) b = mid;
      else a = mid + 1;
    }
    const int i0 = min(K, a * seg), i1 = min(K, i0 + seg);
    const double c0 = base[a];
    double r = 0.0;
    int idx = K - 1;  // (u_j >= 1 only: outside the contract)
    for (int i = i0; i < i1; ++i) {
      r += (double)w[i];
      if (c0 + r > v) {
        idx = i;
        break;
      }
    }
    anc[j] = idx;
  }
  __syncthreads();
  for (int i = lo; i < hi; ++i) w[i] = (float)((double)w[i] / total);
}

// ---------------------------------------------------------------------------------------------------------------- propose
constexpr int TP_THREADS = 256;
constexpr int TP_UN = 4;                             // float4 per thread, stream and span
constexpr int64_t TP_SPAN = 4 * TP_UN * TP_THREADS;  // elements of a row per span
constexpr int64_t TP_GRID = 2048;                    // workgroups while K allows it (256 CUs x 8)

struct TdsCoef {
  float a_t, a_s, c_s, k_x, scale;
  double g;  // (a_s - k_x a_t) c_s / scale
};

__device__ __forceinline__ TdsCoef tds_coef(const float* __restrict__ coef) {
  TdsCoef k = {coef[0], coef[1], coef[2], coef[3], coef[4], 0.0};
  k.g = ((double)k.a_s - (double)k.k_x * (double)k.a_t) * (double)k.c_s / (double)k.scale;
  return k;
}

// one element: x_s, and the weight term z g + g^2 / 2 rounded once to fp32
__device__ __forceinline__ float tds_one(const TdsCoef& k, float xt, float xh, float sc, float z, float& term) {
  const float m = fmaf(k.c_s, sc, xh);
  const float r = fmaf(-k.a_t, m, xt);
  const float xs = fmaf(k.scale, z, fmaf(k.k_x, r, k.a_s * m));
  const double g = k.g * (double)sc;
  term = (float)(g * ((double)z + 0.5 * g));
  return xs;
}

__device__ __forceinline__ float4 tds_four(const TdsCoef& k, float4 xt, float4 xh, float4 sc, float4 z, float4& acc) {
  float4 o, t;
  o.x = tds_one(k, xt.x, xh.x, sc.x, z.x, t.x);
  o.y = tds_one(k, xt.y, xh.y, sc.y, z.y, t.y);
  o.z = tds_one(k, xt.z, xh.z, sc.z, z.z, t.z);
  o.w = tds_one(k, xt.w, xh.w, sc.w, z.w, t.w);
  acc.x += t.x;
  acc.y += t.y;
  acc.z += t.z;
  acc.w += t.w;
  return o;
}

template <bool VEC>
__global__ __launch_bounds__(TP_THREADS) void tds_propose_kernel(const float* __restrict__ x_t, const float* __restrict__ x_hat,
                                                                 const float* __restrict__ score, const float* __restrict__ z,
                                                                 const int64_t* __restrict__ anc, const float* __restrict__ coef,
                                                                 float* __restrict__ x_s, double* __restrict__ work, int64_t K,
                                                                 int64_t N, int chunks) {
  __shared__ double wave_sum[TP_THREADS / AZ_WAVE];
  const int64_t j = blockIdx.x / chunks;
  const int c = (int)(blockIdx.x - j * chunks);
  const int tid = threadIdx.x;
  const int64_t k_raw = anc[j];
  const bool ok = k_raw >= 0 && k_raw < K;
  const int64_t k = ok ? k_raw : 0;
  const TdsCoef q = tds_coef(coef);
  const float* xt = x_t + k * N;
  const float* xh = x_hat + k * N;
  const float* sc = score + k * N;
  const float* zj = z + j * N;
  float* out = x_s + j * N;
  const int64_t spans = (N + TP_SPAN - 1) / TP_SPAN;
  const float nanf_ = __builtin_nanf("");
  double sum = 0.0;

  for (int64_t s = c; s < spans; s += chunks) {
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    if (VEC) {
      const int64_t n4 = N / 4, q0 = s * (TP_SPAN / 4) + tid;
      if ((s + 1) * TP_SPAN <= N) {  // a whole span: every load of the group in flight before the first store
        float4 a[TP_UN], b[TP_UN], d[TP_UN], e[TP_UN];
#pragma unroll
        for (int v = 0; v < TP_UN; ++v) {
          const int64_t p = 4 * (q0 + v * TP_THREADS);
          a[v] = az_ld_stream(xt + p);
          b[v] = az_ld_stream(xh + p);
          d[v] = az_ld_stream(sc + p);
          e[v] = az_ld_stream(zj + p);
        }
#pragma unroll
        for (int v = 0; v < TP_UN; ++v) {
          float4 o = tds_four(q, a[v], b[v], d[v], e[v], acc);
          if (!ok) o = make_float4(nanf_, nanf_, nanf_, nanf_);
          az_st_stream(out + 4 * (q0 + v * TP_THREADS), o);
        }
      } else {  // the row's last span: what is left of it, float4 by float4
        for (int64_t p4 = q0; p4 < n4; p4 += TP_THREADS) {
          const int64_t p = 4 * p4;
          float4 o = tds_four(q, *reinterpret_cast<const float4*>(xt + p), *reinterpret_cast<const float4*>(xh + p),
                              *reinterpret_cast<const float4*>(sc + p), *reinterpret_cast<const float4*>(zj + p), acc);
          if (!ok) o = make_float4(nanf_, nanf_, nanf_, nanf_);
          *reinterpret_cast<float4*>(out + p) = o;
        }
      }
    } else {  // rows not 16-byte aligned: the same spans element by element, accumulator v % 4 for the thread's v-th element
      const int64_t i0 = s * TP_SPAN + tid;
#pragma unroll
      for (int v = 0; v < 4 * TP_UN; ++v) {
        const int64_t i = i0 + (int64_t)v * TP_THREADS;
        if (i < N) {
          float t;
          const float o = tds_one(q, xt[i], xh[i], sc[i], zj[i], t);
          out[i] = ok ? o : nanf_;
          if ((v & 3) == 0) acc.x += t;
          else if ((v & 3) == 1) acc.y += t;
          else if ((v & 3) == 2) acc.z += t;
          else acc.w += t;
        }
      }
    }
    sum += (double)((acc.x + acc.y) + (acc.z + acc.w));
  }

#pragma unroll
  for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
  if ((tid & (AZ_WAVE - 1)) == 0) wave_sum[tid / AZ_WAVE] = sum;
  __syncthreads();
  if (tid == 0) {
    double t = wave_sum[0];
    for (int v = 1; v < TP_THREADS / AZ_WAVE; ++v) t += wave_sum[v];
    work[blockIdx.x] = t;
  }
}

__global__ __launch_bounds__(256) void tds_finish_kernel(const double* __restrict__ work, const int64_t* __restrict__ anc,
                                                         const float* __restrict__ log_p, float* __restrict__ log_w_next,
                                                         int64_t K, int chunks) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= K) return;
  const int64_t k = anc[j];
  if (k < 0 || k >= K) {
    log_w_next[j] = __builtin_nanf("");
    return;
  }
  double t = 0.0;
  for (int c = 0; c < chunks; ++c) t += work[j * chunks + c];
  log_w_next[j] = (float)(-t - (double)log_p[k]);
}

inline bool overlaps(const void* a, const void* b, int64_t bytes) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y + (uintptr_t)bytes && y < x + (uintptr_t)bytes;
}

}  // namespace

extern "C" {

int64_t az_tds_chunks(int64_t K, int64_t N) {
  if (K < 1 || N < 1) return 0;
  const int64_t spans = (N + TP_SPAN - 1) / TP_SPAN;
  int64_t cap = TP_GRID / K;
  if (cap < 1) cap = 1;
  return spans < cap ? spans : cap;
}

int az_tds_resample_f32(const float* log_p, const float* log_w_prev, const float* u, int64_t* ancestors, float* w, int64_t K,
                        az_stream_t stream) {
  AZ_REQUIRE(log_p && u && ancestors && w, AZ_E_NULL);
  AZ_REQUIRE(K >= 1 && K <= RS_MAX_K, AZ_E_SHAPE);
  AZ_REQUIRE((((uintptr_t)log_p | (uintptr_t)log_w_prev | (uintptr_t)u | (uintptr_t)w) & 3u) == 0 &&
                 (((uintptr_t)ancestors) & 7u) == 0,
             AZ_E_ALIGN);
  hipLaunchKernelGGL(tds_resample_kernel, dim3(1), dim3(RS_THREADS), 0, az_s(stream), log_p, log_w_prev, u, ancestors, w, (int)K);
  return az_launch_status();
}

int az_tds_propose_f32(const AzTdsProposeArgs* a, az_stream_t stream) {
  AZ_REQUIRE(a && a->x_t && a->x_hat && a->score && a->z && a->ancestors && a->log_p && a->coef && a->x_s && a->log_w_next &&
                 a->workspace,
             AZ_E_NULL);
  AZ_REQUIRE(a->K >= 1 && a->K <= RS_MAX_K && a->N >= 1 && a->N <= (INT64_MAX / 4) / a->K, AZ_E_SHAPE);
  AZ_REQUIRE(a->chunks == az_tds_chunks(a->K, a->N), AZ_E_SHAPE);
  const int64_t bytes = a->K * a->N * 4;
  // the gather reads other particles' rows: x_s aliases no input
  AZ_REQUIRE(!overlaps(a->x_s, a->x_t, bytes) && !overlaps(a->x_s, a->x_hat, bytes) && !overlaps(a->x_s, a->score, bytes) &&
                 !overlaps(a->x_s, a->z, bytes),
             AZ_E_SHAPE);
  AZ_REQUIRE(AZ_ALIGNED16(a->x_t) && AZ_ALIGNED16(a->x_hat) && AZ_ALIGNED16(a->score) && AZ_ALIGNED16(a->z) &&
                 AZ_ALIGNED16(a->x_s) && AZ_ALIGNED16(a->workspace) && (((uintptr_t)a->ancestors) & 7u) == 0 &&
                 (((uintptr_t)a->log_p | (uintptr_t)a->coef | (uintptr_t)a->log_w_next) & 3u) == 0,
             AZ_E_ALIGN);
  hipStream_t st = az_s(stream);
  const int chunks = (int)a->chunks;
  const dim3 grid((unsigned)(a->K * a->chunks));
  if (a->N % 4 == 0)
    hipLaunchKernelGGL(tds_propose_kernel<true>, grid, dim3(TP_THREADS), 0, st, a->x_t, a->x_hat, a->score, a->z, a->ancestors,
                       a->coef, a->x_s, a->workspace, a->K, a->N, chunks);
  else
    hipLaunchKernelGGL(tds_propose_kernel<false>, grid, dim3(TP_THREADS), 0, st, a->x_t, a->x_hat, a->score, a->z, a->ancestors,
                       a->coef, a->x_s, a->workspace, a->K, a->N, chunks);
  hipLaunchKernelGGL(tds_finish_kernel, dim3((unsigned)((a->K + 255) / 256)), dim3(256), 0, st, a->workspace, a->ancestors,
                     a->log_p, a->log_w_next, a->K, chunks);
  return az_launch_status();
}

}  // extern "C"
