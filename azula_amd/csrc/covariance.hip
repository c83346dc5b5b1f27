// Structured covariance applies (azula/linalg/covariance.py): the per-step products of the seven covariance classes as a few
// streaming passes (include/azula_amd.h, "Covariance applies").  Setup (from_data, capacitances, the r x r eigh of inv / color,
// logdet) stays with the caller.
//
//   * az_cov_scale    y = (k x - u) * h(e) + v, elementwise with e / u / v broadcast across the rows: Isotropic / Diagonal
//                     applies, the spectral core of Full and Kronecker, the posterior factor e / (e + rho) of GaussianDenoiser.
//   * az_cov_project  P[b, j] = sum_f W[f, j] c_f x[b, f]: 512-feature segments, one workgroup per (segment, 64 rank columns)
//                     that walks the rows in passes of 32, staging 64-feature tiles of W and x in LDS; the segments' partial
//                     sums are reduced in a fixed order by a second pass (lane-strided, then the butterfly).  No atomics.
//   * az_cov_expand   y[b, f] = a_f (d_f x[b, f] + s sum_j W[f, j] g_j P[b, j]): 64 features x 32 rows per workgroup, the
//                     rank walked in 64-wide LDS tiles.
//                     Both stage the W tile again for every 32-row pass: W comes from HBM once per launch for batches of up
//                     to 32 rows; larger batches read it again per pass (from L2 / MALL when it fits there).
//   * az_cov_mode     one Kronecker axis: x as [outer, n, inner], y[o, i, k] = sum_m M[i, m] x[o, m, k] with M = Q or Q^T,
//                     64 x 64 output tiles fed from LDS, VALU FMA (the op is bandwidth-bound at these sizes).
// Every output is one dot product summed in a fixed order that depends on the sizes of the factor alone (n, r), never on the
// number of rows: a row's result is the same bits whatever batch it is computed in, and on every run.
#include "common.h"

namespace {

constexpr int CV_SEG = 512;  // features per segment of az_cov_project
constexpr int CV_BT = 32;    // rows per pass of a workgroup (4 waves x 8 accumulators)

template <class T>
__device__ __forceinline__ T cld(const void* p, int f64, int64_t i) {
  return f64 ? (T) static_cast<const double*>(p)[i] : (T) static_cast<const float*>(p)[i];
}

__device__ __forceinline__ float csqrt(float v) { return __fsqrt_rn(v); }
__device__ __forceinline__ double csqrt(double v) { return __dsqrt_rn(v); }

template <class T>
__device__ __forceinline__ T cfma(T a, T b, T c) {
  return sizeof(T) == 8 ? (T)__fma_rn((double)a, (double)b, (double)c) : (T)__fmaf_rn((float)a, (float)b, (float)c);
}

template <class T>
__device__ __forceinline__ T cwave_sum(T v) {  // every lane ends with the same bits
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = v + (T)__shfl_xor(v, o, 64);
  return v;
}

// ------------------------------------------------------------------------------------------------------------- scale
// grid (feature blocks, row blocks), both grid-strided: the feature index needs no division
template <class T>
__global__ __launch_bounds__(256) void cov_scale_kernel(AzCovScaleArgs a) {
  T k = (T)a.k, rho = (T)a.rho;
  if (a.k_dev) k = cld<T>(a.k_dev, a.scalar_dtype, 0);
  if (a.rho_dev) rho = cld<T>(a.rho_dev, a.scalar_dtype, 0);
  const bool scaled = a.k_dev || a.k != 1.0;
  for (int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; f < a.n; f += (int64_t)gridDim.x * blockDim.x) {
    T h = (T)1, uf = (T)0, vf = (T)0;
    if (a.e) {
      const T e = cld<T>(a.e, a.f_dtype, a.e_len == 1 ? 0 : f);
      switch (a.h) {
        case AZ_COV_H_SQRT: h = csqrt(e); break;
        case AZ_COV_H_INV: h = (T)1 / e; break;
        case AZ_COV_H_POSTERIOR: h = e / (e + rho); break;
        default: h = e; break;
      }
    }
    if (a.u) uf = cld<T>(a.u, a.f_dtype, f);
    if (a.v) vf = cld<T>(a.v, a.f_dtype, f);
    for (int64_t b = blockIdx.y; b < a.rows; b += gridDim.y) {
      const int64_t i = b * a.n + f;
      T v = cld<T>(a.x, a.x_dtype, i);
      if (scaled) v = k * v;
      if (a.u) v = v - uf;
      if (a.e) v = v * h;
      if (a.v) v = v + vf;
      static_cast<T*>(a.y)[i] = v;
    }
  }
}

// ----------------------------------------------------------------------------------------------------------- project
// grid (segments, ceil(r / 64)); lane = rank column, wave w = rows w, w + 4, ..., w + 28 of each 32-row pass
template <class T>
__global__ __launch_bounds__(256) void cov_project_kernel(AzCovLowRankArgs a, int64_t nseg) {
  __shared__ T Ws[64][65];
  __shared__ T Xs[CV_BT][65];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int64_t seg = blockIdx.x, j0 = (int64_t)blockIdx.y * 64, j = j0 + lane;
  const int64_t f_beg = seg * CV_SEG, f_end = f_beg + CV_SEG < a.n ? f_beg + CV_SEG : a.n;
  for (int64_t b0 = 0; b0 < a.rows; b0 += CV_BT) {
    T acc[CV_BT / 4];
#pragma unroll
    for (int q = 0; q < CV_BT / 4; ++q) acc[q] = (T)0;
    for (int64_t f0 = f_beg; f0 < f_end; f0 += 64) {
      __syncthreads();
      for (int e = t; e < 64 * 64; e += 256) {
        const int fi = e >> 6, jj = e & 63;
        const int64_t f = f0 + fi, jg = j0 + jj;
        Ws[fi][jj] = (f < f_end && jg < a.r) ? cld<T>(a.W, a.f_dtype, f * a.r + jg) : (T)0;
      }
      for (int e = t; e < CV_BT * 64; e += 256) {
        const int bi = e >> 6, fi = e & 63;
        const int64_t b = b0 + bi, f = f0 + fi;
        T v = (T)0;
        if (b < a.rows && f < f_end) {
          v = cld<T>(a.x, a.x_dtype, b * a.n + f);
          if (a.c) v = cld<T>(a.c, a.f_dtype, f) * v;
        }
        Xs[bi][fi] = v;
      }
      __syncthreads();
#pragma unroll 4
      for (int fi = 0; fi < 64; ++fi) {
        const T wv = Ws[fi][lane];
#pragma unroll
        for (int q = 0; q < CV_BT / 4; ++q) acc[q] = cfma(wv, Xs[w + 4 * q][fi], acc[q]);
      }
    }
    if (j < a.r) {
#pragma unroll
      for (int q = 0; q < CV_BT / 4; ++q) {
        const int64_t b = b0 + w + 4 * q;
        if (b >= a.rows) break;
        if (nseg == 1)
          static_cast<T*>(a.P)[b * a.r + j] = acc[q];
        else
          static_cast<T*>(a.partial)[(seg * a.rows + b) * a.r + j] = acc[q];
      }
    }
  }
}

// one wave per (row, column): P = the segments' partials summed in a fixed order
template <class T>
__global__ __launch_bounds__(256) void cov_project_reduce_kernel(AzCovLowRankArgs a, int64_t nseg) {
  const int64_t gw = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int lane = threadIdx.x & 63;
  if (gw >= a.rows * a.r) return;  // whole waves
  const T* p = static_cast<const T*>(a.partial);
  const int64_t plane = a.rows * a.r;
  T acc = (T)0;
  for (int64_t s = lane; s < nseg; s += 64) acc = acc + p[s * plane + gw];
  acc = cwave_sum(acc);
  if (lane == 0) static_cast<T*>(a.P)[gw] = acc;
}

// ------------------------------------------------------------------------------------------------------------ expand
// grid (ceil(n / 64), ceil(rows / 32)); lane = feature, wave w = rows w, w + 4, ...
template <class T>
__global__ __launch_bounds__(256) void cov_expand_kernel(AzCovLowRankArgs a) {
  __shared__ T Ws[64][65];
  __shared__ T Ps[CV_BT][65];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int64_t f0 = (int64_t)blockIdx.x * 64, f = f0 + lane, b0 = (int64_t)blockIdx.y * CV_BT;
  T acc[CV_BT / 4];
#pragma unroll
  for (int q = 0; q < CV_BT / 4; ++q) acc[q] = (T)0;
  for (int64_t j0 = 0; j0 < a.r; j0 += 64) {
    __syncthreads();
    for (int e = t; e < 64 * 64; e += 256) {
      const int fi = e >> 6, jj = e & 63;
      const int64_t fg = f0 + fi, jg = j0 + jj;
      Ws[fi][jj] = (fg < a.n && jg < a.r) ? cld<T>(a.W, a.f_dtype, fg * a.r + jg) : (T)0;
    }
    for (int e = t; e < CV_BT * 64; e += 256) {
      const int bi = e >> 6, jj = e & 63;
      const int64_t b = b0 + bi, jg = j0 + jj;
      T v = (T)0;
      if (b < a.rows && jg < a.r) {
        v = static_cast<const T*>(a.P)[b * a.r + jg];
        if (a.g) v = cld<T>(a.g, a.f_dtype, jg) * v;
      }
      Ps[bi][jj] = v;
    }
    __syncthreads();
#pragma unroll 4
    for (int jj = 0; jj < 64; ++jj) {
      const T wv = Ws[lane][jj];
#pragma unroll
      for (int q = 0; q < CV_BT / 4; ++q) acc[q] = cfma(wv, Ps[w + 4 * q][jj], acc[q]);
    }
  }
  if (f >= a.n) return;
  const T s = (T)a.s;
  const T av = a.a ? cld<T>(a.a, a.f_dtype, f) : (T)1;
  const T dv = a.d ? cld<T>(a.d, a.f_dtype, f) : (T)a.d0;
#pragma unroll
  for (int q = 0; q < CV_BT / 4; ++q) {
    const int64_t b = b0 + w + 4 * q;
    if (b >= a.rows) break;
    T v = s * acc[q];
    if (a.x) v = dv * cld<T>(a.x, a.x_dtype, b * a.n + f) + v;
    if (a.a) v = av * v;
    static_cast<T*>(a.y)[b * a.n + f] = v;
  }
}

// -------------------------------------------------------------------------------------------------------------- mode
// columns c = (o, k) flattened, o = c / inner; grid (ceil(outer * inner / 64), ceil(n / 64)); lane = column, wave w = output
// indices i0 + 16 w + [0, 16)
template <class T>
__global__ __launch_bounds__(256) void cov_mode_kernel(AzCovModeArgs a) {
  __shared__ T Ms[64][65];
  __shared__ T Xs[64][65];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int64_t cols = a.outer * a.inner, n = a.n, inner = a.inner;
  const int64_t c0 = (int64_t)blockIdx.x * 64, i0 = (int64_t)blockIdx.y * 64;
  const bool wide_inner = inner >= 64;
  T acc[16];
#pragma unroll
  for (int q = 0; q < 16; ++q) acc[q] = (T)0;
  for (int64_t m0 = 0; m0 < n; m0 += 64) {
    __syncthreads();
    for (int e = t; e < 64 * 64; e += 256) {
      const int mi = wide_inner ? e >> 6 : e & 63, ci = wide_inner ? e & 63 : e >> 6;
      const int64_t c = c0 + ci, m = m0 + mi;
      T v = (T)0;
      if (c < cols && m < n) {
        const int64_t o = c / inner, k = c - o * inner;
        v = cld<T>(a.x, a.x_dtype, (o * n + m) * inner + k);
      }
      Xs[mi][ci] = v;
    }
    for (int e = t; e < 64 * 64; e += 256) {
      const int ii = a.transpose ? e & 63 : e >> 6, mi = a.transpose ? e >> 6 : e & 63;
      const int64_t i = i0 + ii, m = m0 + mi;
      T v = (T)0;
      if (i < n && m < n) v = cld<T>(a.Q, a.f_dtype, a.transpose ? m * n + i : i * n + m);
      Ms[ii][mi] = v;
    }
    __syncthreads();
#pragma unroll 4
    for (int mi = 0; mi < 64; ++mi) {
      const T xv = Xs[mi][lane];
#pragma unroll
      for (int q = 0; q < 16; ++q) acc[q] = cfma(Ms[16 * w + q][mi], xv, acc[q]);
    }
  }
  const int64_t c = c0 + lane;
  if (c >= cols) return;
  const int64_t o = c / inner, k = c - o * inner;
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const int64_t i = i0 + 16 * w + q;
    if (i < n) static_cast<T*>(a.y)[(o * n + i) * inner + k] = acc[q];
  }
}

// ------------------------------------------------------------------------------------------------------------ launch
bool dtype_ok(int32_t d) { return d == 0 || d == 1; }
// the output dtype is torch's promotion of the operand dtypes
bool promoted(int32_t x, int32_t f, int32_t out) { return dtype_ok(x) && dtype_ok(f) && out == (x > f ? x : f); }
int64_t segments(int64_t n) { return (n + CV_SEG - 1) / CV_SEG; }

template <class F>
int dispatch_out(int32_t out, F&& f) {
  return out == 1 ? f(double()) : f(float());
}

int check_lowrank(const AzCovLowRankArgs* a) {
  AZ_REQUIRE(a, AZ_E_NULL);
  AZ_REQUIRE(a->rows > 0 && a->n > 0 && a->r > 0, AZ_E_SHAPE);
  AZ_REQUIRE(promoted(a->x_dtype, a->f_dtype, a->out_dtype), AZ_E_UNSUPPORTED);
  AZ_REQUIRE(a->W && a->P, AZ_E_NULL);
  AZ_REQUIRE((a->r + 63) / 64 <= 65535, AZ_E_SHAPE);
  return AZ_OK;
}

}  // namespace

extern "C" {

int64_t az_cov_segments(int64_t n) { return n > 0 ? segments(n) : 0; }

int az_cov_scale(const AzCovScaleArgs* a, az_stream_t stream) {
  AZ_REQUIRE(a, AZ_E_NULL);
  AZ_REQUIRE(a->x && a->y, AZ_E_NULL);
  AZ_REQUIRE(a->rows > 0 && a->n > 0, AZ_E_SHAPE);
  AZ_REQUIRE(!a->e || a->e_len == 1 || a->e_len == a->n, AZ_E_SHAPE);
  AZ_REQUIRE(a->h >= AZ_COV_H_IDENTITY && a->h <= AZ_COV_H_POSTERIOR, AZ_E_UNSUPPORTED);
  AZ_REQUIRE(promoted(a->x_dtype, a->f_dtype, a->out_dtype) && dtype_ok(a->scalar_dtype), AZ_E_UNSUPPORTED);
  const int64_t total = a->rows * a->n;
  AZ_REQUIRE(total / a->n == a->rows, AZ_E_SHAPE);
  int64_t fblocks = (a->n + 255) / 256, rblocks = a->rows;
  if (fblocks > 65536) fblocks = 65536;  // both grid-strided
  if (rblocks > 65535) rblocks = 65535;
  hipStream_t st = az_s(stream);
  return dispatch_out(a->out_dtype, [&](auto t) {
    hipLaunchKernelGGL((cov_scale_kernel<decltype(t)>), dim3((unsigned)fblocks, (unsigned)rblocks), dim3(256), 0, st, *a);
    return az_launch_status();
  });
}

int az_cov_project(const AzCovLowRankArgs* a, az_stream_t stream) {
  const int rc = check_lowrank(a);
  if (rc != AZ_OK) return rc;
  AZ_REQUIRE(a->x, AZ_E_NULL);
  const int64_t nseg = segments(a->n);
  AZ_REQUIRE(nseg == 1 || a->partial, AZ_E_NULL);
  AZ_REQUIRE(nseg <= (int64_t)0x7FFFFFFF, AZ_E_SHAPE);
  const int64_t rblocks = (a->rows * a->r * 64 + 255) / 256;
  AZ_REQUIRE(rblocks <= (int64_t)0x7FFFFFFF, AZ_E_SHAPE);
  hipStream_t st = az_s(stream);
  return dispatch_out(a->out_dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL((cov_project_kernel<T>), dim3((unsigned)nseg, (unsigned)((a->r + 63) / 64)), dim3(256), 0, st, *a, nseg);
    if (nseg > 1) hipLaunchKernelGGL((cov_project_reduce_kernel<T>), dim3((unsigned)rblocks), dim3(256), 0, st, *a, nseg);
    return az_launch_status();
  });
}

int az_cov_expand(const AzCovLowRankArgs* a, az_stream_t stream) {
  const int rc = check_lowrank(a);
  if (rc != AZ_OK) return rc;
  AZ_REQUIRE(a->y, AZ_E_NULL);
  const int64_t fblocks = (a->n + 63) / 64, bblocks = (a->rows + CV_BT - 1) / CV_BT;
  AZ_REQUIRE(fblocks <= (int64_t)0x7FFFFFFF && bblocks <= 65535, AZ_E_SHAPE);
  hipStream_t st = az_s(stream);
  return dispatch_out(a->out_dtype, [&](auto t) {
    hipLaunchKernelGGL((cov_expand_kernel<decltype(t)>), dim3((unsigned)fblocks, (unsigned)bblocks), dim3(256), 0, st, *a);
    return az_launch_status();
  });
}

int az_cov_mode(const AzCovModeArgs* a, az_stream_t stream) {
  AZ_REQUIRE(a, AZ_E_NULL);
  AZ_REQUIRE(a->x && a->Q && a->y, AZ_E_NULL);
  AZ_REQUIRE(a->x != a->y, AZ_E_UNSUPPORTED);
  AZ_REQUIRE(a->outer > 0 && a->n > 0 && a->inner > 0, AZ_E_SHAPE);
  AZ_REQUIRE(promoted(a->x_dtype, a->f_dtype, a->out_dtype), AZ_E_UNSUPPORTED);
  const int64_t cblocks = (a->outer * a->inner + 63) / 64, iblocks = (a->n + 63) / 64;
  AZ_REQUIRE(cblocks <= (int64_t)0x7FFFFFFF && iblocks <= 65535, AZ_E_SHAPE);
  hipStream_t st = az_s(stream);
  return dispatch_out(a->out_dtype, [&](auto t) {
    hipLaunchKernelGGL((cov_mode_kernel<decltype(t)>), dim3((unsigned)cblocks, (unsigned)iblocks), dim3(256), 0, st, *a);
    return az_launch_status();
  });
}

}  // extern "C"
