// Krylov solvers (azula/linalg/solve.py): the per-iteration arithmetic of CG and GMRES as a few streaming passes per
// iteration; the caller runs the operator A between the entries (include/azula_amd.h, "Krylov solvers").
//
// Every row of b is an independent system (the reference's "...i,...i" dot products reduce over the last dimension).  Work
// is organised in waves: one wave owns one SEGMENT of a row, lane l holding elements seg * 64E + 64k + l, k < E.
//   * short rows (dim <= 1024): one segment per row, E = the power of two that covers it; every entry is ONE pass, its
//     dependent reductions wave butterflies in registers (CG step: pAp -> alpha -> x, r -> rr_ -> beta -> p in one launch);
//   * long rows: 1024-element segments (E = 16); a reduction writes one partial per segment and the next pass reduces the
//     row's partials in a fixed order (lane-strided sum, then the butterfly), each wave of the row redundantly, so every
//     wave sees the same bits.  No atomics, no cross-workgroup waiting.
// The regime and E depend on dim alone, so a row's result never depends on the batch or the grid.
#include "common.h"

namespace {

constexpr int KR_SHORT_MAX = 1024;  // longest row of the one-wave regime
constexpr int KR_SEG_E = 16;        // elements per lane of a long-row segment (1024 per wave)

// separately rounded arithmetic (the torch op sequence rounds every op; -ffp-contract never fuses these)
__device__ __forceinline__ float kmul(float a, float b) { return __fmul_rn(a, b); }
__device__ __forceinline__ double kmul(double a, double b) { return __dmul_rn(a, b); }
__device__ __forceinline__ float kadd(float a, float b) { return __fadd_rn(a, b); }
__device__ __forceinline__ double kadd(double a, double b) { return __dadd_rn(a, b); }
__device__ __forceinline__ float ksub(float a, float b) { return __fsub_rn(a, b); }
__device__ __forceinline__ double ksub(double a, double b) { return __dsub_rn(a, b); }
__device__ __forceinline__ float kdiv(float a, float b) { return __fdiv_rn(a, b); }
__device__ __forceinline__ double kdiv(double a, double b) { return __ddiv_rn(a, b); }
__device__ __forceinline__ float ksqrt(float a) { return __fsqrt_rn(a); }
__device__ __forceinline__ double ksqrt(double a) { return __dsqrt_rn(a); }

template <class T>
__device__ __forceinline__ T keps() {
  return sizeof(T) == 8 ? (T)2.220446049250313080847e-16 : (T)1.1920928955078125e-07f;  // torch.finfo(dtype).eps
}
// torch.clip(v, min=eps): NaN stays NaN
template <class T>
__device__ __forceinline__ T kclip(T v) {
  return v < keps<T>() ? keps<T>() : v;
}

template <class T>
__device__ __forceinline__ T kwave_sum(T v) {  // every lane ends with the same bits (a + b == b + a)
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = kadd(v, (T)__shfl_xor(v, o, 64));
  return v;
}

// element i of a tensor whose dtype is a run-time flag (0 = fp32, 1 = fp64), converted to T as Tensor.to(dtype) does
template <class T>
__device__ __forceinline__ T kld(const void* p, int f64, int64_t i) {
  return f64 ? (T) static_cast<const double*>(p)[i] : (T) static_cast<const float*>(p)[i];
}

// the wave's row / segment / lane; false for the waves past the last row (whole waves: no barrier follows)
struct KWave {
  int64_t row, seg;
  int lane;
};
__device__ __forceinline__ bool kwave(int64_t rows, int64_t nseg, KWave& w) {
  const int64_t gw = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  w.lane = threadIdx.x & 63;
  w.row = gw / nseg;
  w.seg = gw - w.row * nseg;
  return w.row < rows;
}

// the row's reduced value of partial slot `slot` (fixed order: lane-strided, then the butterfly)
template <class T>
__device__ __forceinline__ T kreduce(const void* partial, int slot, int64_t rows, int64_t row, int64_t nseg, int lane) {
  const T* p = static_cast<const T*>(partial) + ((int64_t)slot * rows + row) * nseg;
  T acc = (T)0;
  for (int64_t s = lane; s < nseg; s += 64) acc = kadd(acc, p[s]);
  return kwave_sum(acc);
}
template <class T>
__device__ __forceinline__ void kput_partial(void* partial, int slot, int64_t rows, const KWave& w, int64_t nseg, T v) {
  if (w.lane == 0) static_cast<T*>(partial)[((int64_t)slot * rows + w.row) * nseg + w.seg] = v;
}

// element index (within the row) of lane element k, and whether it exists
template <int E>
__device__ __forceinline__ int64_t kidx(const KWave& w, int k) {
  return w.seg * (64 * E) + 64 * k + w.lane;
}

// ------------------------------------------------------------------------------------------------------------------ CG
// init (solve.py:51-61).  phase 2: short rows, rr in the same pass; phase 0: long rows, partials of r.r; phase 1: reduce them.
template <class T, class U, int E>
__global__ __launch_bounds__(256) void cg_init_kernel(AzCgArgs a, int64_t nseg, int phase) {
  KWave w;
  if (!kwave(a.rows, phase == 1 ? 1 : nseg, w)) return;
  if (phase == 1) {
    const T s = kreduce<T>(a.partial, 0, a.rows, w.row, nseg, w.lane);
    if (w.lane == 0) static_cast<T*>(a.rr_out)[w.row] = s;
    return;
  }
  const int64_t base = w.row * a.dim;
  T acc = (T)0;
#pragma unroll
  for (int k = 0; k < E; ++k) {
    const int64_t e = kidx<E>(w, k);
    if (e < a.dim) {
      const T r = kld<T>(a.r0, a.in_dtype, base + e);
      static_cast<T*>(a.x)[base + e] = a.x0 ? kld<T>(a.x0, a.io_dtype, base + e) : (T)0;
      static_cast<T*>(a.r)[base + e] = r;
      static_cast<T*>(a.p)[base + e] = r;
      static_cast<U*>(a.p_io)[base + e] = (U)r;
      acc = kadd(acc, kmul(r, r));
    }
  }
  if (phase == 0) return kput_partial(a.partial, 0, a.rows, w, nseg, kwave_sum(acc));
  const T rr = kwave_sum(acc);
  if (w.lane == 0) static_cast<T*>(a.rr_out)[w.row] = rr;
}

// one iteration on a short row (solve.py:63-73): every reduction in registers, one pass
template <class T, class U, int E>
__global__ __launch_bounds__(256) void cg_step_short_kernel(AzCgArgs a) {
  KWave w;
  if (!kwave(a.rows, 1, w)) return;
  const int64_t base = w.row * a.dim;
  T ap[E], p[E], r[E];
  T acc = (T)0;
#pragma unroll
  for (int k = 0; k < E; ++k) {
    const int64_t e = kidx<E>(w, k);
    const bool ok = e < a.dim;
    ap[k] = ok ? kld<T>(a.Ap, a.in_dtype, base + e) : (T)0;
    p[k] = ok ? static_cast<const T*>(a.p)[base + e] : (T)0;
    if (ok) acc = kadd(acc, kmul(p[k], ap[k]));
  }
  const T rr = static_cast<const T*>(a.rr)[w.row];
  const T alpha = kdiv(rr, kclip(kwave_sum(acc)));
  const bool last = a.out != nullptr;
  acc = (T)0;
#pragma unroll
  for (int k = 0; k < E; ++k) {
    const int64_t e = kidx<E>(w, k);
    if (e < a.dim) {
      const T x = kadd(static_cast<const T*>(a.x)[base + e], kmul(alpha, p[k]));
      r[k] = ksub(static_cast<const T*>(a.r)[base + e], kmul(alpha, ap[k]));
      if (last) {
        static_cast<U*>(a.out)[base + e] = (U)x;
      } else {
        static_cast<T*>(a.x)[base + e] = x;
        static_cast<T*>(a.r)[base + e] = r[k];
        acc = kadd(acc, kmul(r[k], r[k]));
      }
    }
  }
  if (last) return;  // the reference's last rr_ / beta / p_ are never read
  const T rr_ = kwave_sum(acc);
  const T beta = kdiv(rr_, kclip(rr));
#pragma unroll
  for (int k = 0; k < E; ++k) {
    const int64_t e = kidx<E>(w, k);
    if (e < a.dim) {
      const T pn = kadd(r[k], kmul(beta, p[k]));
      static_cast<T*>(a.p)[base + e] = pn;
      static_cast<U*>(a.p_io)[base + e] = (U)pn;
    }
  }
  if (w.lane == 0) static_cast<T*>(a.rr_out)[w.row] = rr_;
}

// one iteration on long rows, three passes: 0 = partials of p.Ap; 1 = alpha, x, r (or x.to(b)), partials of r_.r_;
// 2 = beta, p, p_io, rr_out
template <class T, class U>
__global__ __launch_bounds__(256) void cg_step_long_kernel(AzCgArgs a, int64_t nseg, int pass) {
  constexpr int E = KR_SEG_E;
  KWave w;
  if (!kwave(a.rows, nseg, w)) return;
  const int64_t base = w.row * a.dim;
  T acc = (T)0;
  if (pass == 0) {
#pragma unroll
    for (int k = 0; k < E; ++k) {
      const int64_t e = kidx<E>(w, k);
      if (e < a.dim) acc = kadd(acc, kmul(static_cast<const T*>(a.p)[base + e], kld<T>(a.Ap, a.in_dtype, base + e)));
    }
    return kput_partial(a.partial, 0, a.rows, w, nseg, kwave_sum(acc));
  }
  const T rr = static_cast<const T*>(a.rr)[w.row];
  if (pass == 1) {
    const T alpha = kdiv(rr, kclip(kreduce<T>(a.partial, 0, a.rows, w.row, nseg, w.lane)));
    const bool last = a.out != nullptr;
#pragma unroll
    for (int k = 0; k < E; ++k) {
      const int64_t e = kidx<E>(w, k);
      if (e < a.dim) {
        const T p = static_cast<const T*>(a.p)[base + e];
        const T x = kadd(static_cast<const T*>(a.x)[base + e], kmul(alpha, p));
        const T r = ksub(static_cast<const T*>(a.r)[base + e], kmul(alpha, kld<T>(a.Ap, a.in_dtype, base + e)));
        if (last) {
          static_cast<U*>(a.out)[base + e] = (U)x;
        } else {
          static_cast<T*>(a.x)[base + e] = x;
          static_cast<T*>(a.r)[base + e] = r;
          acc = kadd(acc, kmul(r, r));
        }
      }
    }
    if (!last) kput_partial(a.partial, 1, a.rows, w, nseg, kwave_sum(acc));
    return;
  }
  const T rr_ = kreduce<T>(a.partial, 1, a.rows, w.row, nseg, w.lane);
  const T beta = kdiv(rr_, kclip(rr));
#pragma unroll
  for (int k = 0; k < E; ++k) {
    const int64_t e = kidx<E>(w, k);
    if (e < a.dim) {
      const T pn = kadd(static_cast<const T*>(a.r)[base + e], kmul(beta, static_cast<const T*>(a.p)[base + e]));
      static_cast<T*>(a.p)[base + e] = pn;
      static_cast<U*>(a.p_io)[base + e] = (U)pn;
    }
  }
  if (w.seg == 0 && w.lane == 0) static_cast<T*>(a.rr_out)[w.row] = rr_;
}

// ------------------------------------------------------------------------------------------------------------------ GMRES
template <class T>
__device__ __forceinline__ T* kH(const AzGmresArgs& a, int64_t row, int i, int j) {
  return static_cast<T*>(a.H) + (row * (a.iterations + 1) + i) * a.iterations + j;
}
template <class T>
__device__ __forceinline__ T* kV(const AzGmresArgs& a, int i, int64_t row) {
  return static_cast<T*>(a.V) + ((int64_t)i * a.rows + row) * a.dim;
}

// solve.py:152-162 for one row, one thread: the previous rotations on column j, the new rotation, the B update
template <class T>
__device__ void gmres_rotate_row(const AzGmresArgs& a, int64_t row, int j) {
  T* cs = static_cast<T*>(a.cs) + row * a.iterations;
  T* ss = static_cast<T*>(a.ss) + row * a.iterations;
  T* B = static_cast<T*>(a.B) + row * (a.iterations + 1);
  for (int i = 0; i < j; ++i) {
    const T hi = *kH<T>(a, row, i, j), hn = *kH<T>(a, row, i + 1, j);
    *kH<T>(a, row, i + 1, j) = kadd(kmul(cs[i], hn), kmul(ss[i], hi));
    *kH<T>(a, row, i, j) = ksub(kmul(cs[i], hi), kmul(ss[i], hn));
  }
  const T hjj = *kH<T>(a, row, j, j), hn = *kH<T>(a, row, j + 1, j);
  const T c = kclip(ksqrt(kadd(kmul(hjj, hjj), kmul(hn, hn))));
  const T cj = kdiv(hjj, c), sj = kdiv(-hn, c);
  cs[j] = cj;
  ss[j] = sj;
  *kH<T>(a, row, j, j) = ksub(kmul(cj, hjj), kmul(sj, hn));
  const T bj = B[j];
  B[j + 1] = kmul(sj, bj);
  B[j] = kmul(cj, bj);
}

// init (solve.py:113-137).  phase 2: short rows, one pass; phase 0: long rows, partials of r.r; phase 1: normalise.
template <class T, class U, int E>
__global__ __launch_bounds__(256) void gmres_init_kernel(AzGmresArgs a, int64_t nseg, int phase) {
  KWave w;
  if (!kwave(a.rows, nseg, w)) return;
  const int64_t base = w.row * a.dim;
  T r[E];
  T acc = (T)0;
#pragma unroll
  for (int k = 0; k < E; ++k) {
    const int64_t e = kidx<E>(w, k);
    r[k] = e < a.dim ? kld<T>(a.r0, a.in_dtype, base + e) : (T)0;
    if (e < a.dim) acc = kadd(acc, kmul(r[k], r[k]));
  }
  if (phase == 0) return kput_partial(a.partial, 0, a.rows, w, nseg, kwave_sum(acc));
  const T norm = ksqrt(phase == 1 ? kreduce<T>(a.partial, 0, a.rows, w.row, nseg, w.lane) : kwave_sum(acc));
  const T d = kclip(norm);
  T* v = kV<T>(a, 0, w.row);
#pragma unroll
  for (int k = 0; k < E; ++k) {
    const int64_t e = kidx<E>(w, k);
    if (e < a.dim) {
      const T q = kdiv(r[k], d);
      v[e] = q;
      static_cast<U*>(a.v_io)[base + e] = (U)q;
    }
  }
  if (w.seg == 0 && w.lane == 0) static_cast<T*>(a.B)[w.row * (a.iterations + 1)] = norm;
}

// Arnoldi iteration j on a short row (solve.py:139-166) in one pass: MGS against V_0..V_j in registers, normalise, rotate
template <class T, class U, int E>
__global__ __launch_bounds__(256) void gmres_arnoldi_short_kernel(AzGmresArgs a) {
  KWave w;
  if (!kwave(a.rows, 1, w)) return;
  const int j = a.j;
  const int64_t base = w.row * a.dim;
  T x[E];
#pragma unroll
  for (int k = 0; k < E; ++k) {
    const int64_t e = kidx<E>(w, k);
    x[k] = e < a.dim ? kld<T>(a.w, a.in_dtype, base + e) : (T)0;
  }
  for (int i = 0; i <= j; ++i) {
    const T* v = kV<T>(a, i, w.row);
    T vi[E];
    T acc = (T)0;
#pragma unroll
    for (int k = 0; k < E; ++k) {
      const int64_t e = kidx<E>(w, k);
      vi[k] = e < a.dim ? v[e] : (T)0;
      if (e < a.dim) acc = kadd(acc, kmul(x[k], vi[k]));
    }
    const T h = kwave_sum(acc);
#pragma unroll
    for (int k = 0; k < E; ++k) x[k] = ksub(x[k], kmul(h, vi[k]));
    if (w.lane == 0) *kH<T>(a, w.row, i, j) = h;
  }
  T acc = (T)0;
#pragma unroll
  for (int k = 0; k < E; ++k)
    if (kidx<E>(w, k) < a.dim) acc = kadd(acc, kmul(x[k], x[k]));
  const T norm = ksqrt(kwave_sum(acc));
  if (j + 1 < a.iterations) {  // V_iterations is never read
    const T d = kclip(norm);
    T* v = kV<T>(a, j + 1, w.row);
#pragma unroll
    for (int k = 0; k < E; ++k) {
      const int64_t e = kidx<E>(w, k);
      if (e < a.dim) {
        const T q = kdiv(x[k], d);
        v[e] = q;
        static_cast<U*>(a.v_io)[base + e] = (U)q;
      }
    }
  }
  if (w.lane == 0) {
    *kH<T>(a, w.row, j + 1, j) = norm;
    gmres_rotate_row<T>(a, w.row, j);
  }
}

// Arnoldi iteration j on long rows: pass i <= j subtracts h_{i-1} V_{i-1} (h from slot i - 1) and writes the partials of
// w.V_i to slot i; pass j + 1 subtracts h_j V_j and writes the partials of w.w to slot j + 1.
template <class T>
__global__ __launch_bounds__(256) void gmres_mgs_long_kernel(AzGmresArgs a, int64_t nseg, int pass) {
  constexpr int E = KR_SEG_E;
  KWave w;
  if (!kwave(a.rows, nseg, w)) return;
  const int64_t base = w.row * a.dim;
  T* work = static_cast<T*>(a.work) + base;
  const T h = pass > 0 ? kreduce<T>(a.partial, pass - 1, a.rows, w.row, nseg, w.lane) : (T)0;
  const T* vprev = pass > 0 ? kV<T>(a, pass - 1, w.row) : nullptr;
  const T* vdot = pass <= a.j ? kV<T>(a, pass, w.row) : nullptr;
  T acc = (T)0;
#pragma unroll
  for (int k = 0; k < E; ++k) {
    const int64_t e = kidx<E>(w, k);
    if (e < a.dim) {
      T x = pass == 0 ? kld<T>(a.w, a.in_dtype, base + e) : ksub(work[e], kmul(h, vprev[e]));
      work[e] = x;
      acc = kadd(acc, kmul(x, vdot ? vdot[e] : x));
    }
  }
  kput_partial(a.partial, pass, a.rows, w, nseg, kwave_sum(acc));
}

// the last pass of a long-row Arnoldi iteration: V_{j+1} = w / clip(norm) and v_io (not on the last iteration); the
// segment-0 wave of each row reduces the j + 2 slots into H[:, j] and rotates
template <class T, class U>
__global__ __launch_bounds__(256) void gmres_normalize_long_kernel(AzGmresArgs a, int64_t nseg) {
  constexpr int E = KR_SEG_E;
  KWave w;
  if (!kwave(a.rows, nseg, w)) return;
  const int j = a.j;
  const T norm = ksqrt(kreduce<T>(a.partial, j + 1, a.rows, w.row, nseg, w.lane));
  if (j + 1 < a.iterations) {
    const int64_t base = w.row * a.dim;
    const T d = kclip(norm);
    const T* work = static_cast<const T*>(a.work) + base;
    T* v = kV<T>(a, j + 1, w.row);
#pragma unroll
    for (int k = 0; k < E; ++k) {
      const int64_t e = kidx<E>(w, k);
      if (e < a.dim) {
        const T q = kdiv(work[e], d);
        v[e] = q;
        static_cast<U*>(a.v_io)[base + e] = (U)q;
      }
    }
  }
  if (w.seg != 0) return;
  for (int i = 0; i <= j; ++i) {
    const T h = kreduce<T>(a.partial, i, a.rows, w.row, nseg, w.lane);
    if (w.lane == 0) *kH<T>(a, w.row, i, j) = h;
  }
  if (w.lane == 0) {
    *kH<T>(a, w.row, j + 1, j) = norm;
    gmres_rotate_row<T>(a, w.row, j);
  }
}

// solve.py:174-178: (H + eps I) y = B, upper triangular, one thread per row; y overwrites B
template <class T>
__global__ __launch_bounds__(256) void gmres_backsolve_kernel(AzGmresArgs a) {
  const int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= a.rows) return;
  const int n = a.iterations;
  T* B = static_cast<T*>(a.B) + row * (n + 1);
  for (int k = n - 1; k >= 0; --k) {
    T s = B[k];
    for (int m = n - 1; m > k; --m) s = ksub(s, kmul(*kH<T>(a, row, k, m), B[m]));
    B[k] = kdiv(s, kadd(*kH<T>(a, row, k, k), keps<T>()));
  }
}

// solve.py:180-185: x = x0 + sum_i V_i y_i, written as x.to(b)
template <class T, class U, int E>
__global__ __launch_bounds__(256) void gmres_combine_kernel(AzGmresArgs a, int64_t nseg) {
  KWave w;
  if (!kwave(a.rows, nseg, w)) return;
  const int64_t base = w.row * a.dim;
  const T* y = static_cast<const T*>(a.B) + w.row * (a.iterations + 1);
  T x[E];
#pragma unroll
  for (int k = 0; k < E; ++k) x[k] = (T)0;
  for (int i = 0; i < a.iterations; ++i) {
    const T yi = y[i];
    const T* v = kV<T>(a, i, w.row);
#pragma unroll
    for (int k = 0; k < E; ++k) {
      const int64_t e = kidx<E>(w, k);
      if (e < a.dim) x[k] = kadd(x[k], kmul(v[e], yi));
    }
  }
#pragma unroll
  for (int k = 0; k < E; ++k) {
    const int64_t e = kidx<E>(w, k);
    if (e < a.dim) {
      const T s = a.x0 ? kadd(kld<T>(a.x0, a.io_dtype, base + e), x[k]) : x[k];
      static_cast<U*>(a.out)[base + e] = (U)s;
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------ launch
int64_t segments(int64_t dim) { return dim <= KR_SHORT_MAX ? 1 : (dim + 64 * KR_SEG_E - 1) / (64 * KR_SEG_E); }
int short_e(int64_t dim) {  // elements per lane of the one-wave regime
  int e = 1;
  while (64 * e < dim) e *= 2;
  return e;
}
bool grid_for(int64_t rows, int64_t nseg, dim3& grid) {  // 4 waves per workgroup
  const int64_t blocks = (rows * nseg + 3) / 4;
  if (blocks < 1 || blocks > (int64_t)0x7FFFFFFF) return false;
  grid = dim3((unsigned)blocks);
  return true;
}

// state / io dtype pairs: (fp64, fp32), (fp32, fp32), (fp64, fp64)
template <class F>
int dispatch_types(int state, int io, F&& f) {
  if (state == 1 && io == 0) return f(double(), float());
  if (state == 0 && io == 0) return f(float(), float());
  if (state == 1 && io == 1) return f(double(), double());
  return AZ_E_UNSUPPORTED;
}
template <class F>
int dispatch_e(int e, F&& f) {
  switch (e) {
    case 1: return f(std::integral_constant<int, 1>());
    case 2: return f(std::integral_constant<int, 2>());
    case 4: return f(std::integral_constant<int, 4>());
    case 8: return f(std::integral_constant<int, 8>());
    default: return f(std::integral_constant<int, 16>());
  }
}

bool dtype_ok(int32_t d) { return d == 0 || d == 1; }

int check_cg(const AzCgArgs* a) {
  AZ_REQUIRE(a, AZ_E_NULL);
  AZ_REQUIRE(a->rows > 0 && a->dim > 0, AZ_E_SHAPE);
  AZ_REQUIRE(dtype_ok(a->state_dtype) && dtype_ok(a->io_dtype) && dtype_ok(a->in_dtype), AZ_E_UNSUPPORTED);
  AZ_REQUIRE(!(a->io_dtype == 1 && a->state_dtype == 0), AZ_E_UNSUPPORTED);
  AZ_REQUIRE(a->x && a->r && a->p && a->rr_out, AZ_E_NULL);
  AZ_REQUIRE(segments(a->dim) == 1 || a->partial, AZ_E_NULL);
  return AZ_OK;
}

int check_gmres(const AzGmresArgs* a) {
  AZ_REQUIRE(a, AZ_E_NULL);
  AZ_REQUIRE(a->rows > 0 && a->dim > 0, AZ_E_SHAPE);
  AZ_REQUIRE(a->iterations >= 1 && a->iterations <= AZ_KRYLOV_GMRES_MAX, AZ_E_UNSUPPORTED);
  AZ_REQUIRE(dtype_ok(a->state_dtype) && dtype_ok(a->io_dtype) && dtype_ok(a->in_dtype), AZ_E_UNSUPPORTED);
  AZ_REQUIRE(!(a->io_dtype == 1 && a->state_dtype == 0), AZ_E_UNSUPPORTED);
  AZ_REQUIRE(a->V && a->H && a->cs && a->ss && a->B, AZ_E_NULL);
  AZ_REQUIRE(segments(a->dim) == 1 || (a->partial && a->work), AZ_E_NULL);
  return AZ_OK;
}

}  // namespace

extern "C" {

int64_t az_krylov_segments(int64_t dim) { return dim > 0 ? segments(dim) : 0; }

int az_cg_init(const AzCgArgs* a, az_stream_t stream) {
  const int rc = check_cg(a);
  if (rc != AZ_OK) return rc;
  AZ_REQUIRE(a->r0 && a->p_io, AZ_E_NULL);
  const int64_t nseg = segments(a->dim);
  dim3 grid, grid1;
  AZ_REQUIRE(grid_for(a->rows, nseg, grid) && grid_for(a->rows, 1, grid1), AZ_E_SHAPE);
  hipStream_t st = az_s(stream);
  return dispatch_types(a->state_dtype, a->io_dtype, [&](auto t, auto u) {
    using T = decltype(t);
    using U = decltype(u);
    if (nseg == 1)
      return dispatch_e(short_e(a->dim), [&](auto e) {
        hipLaunchKernelGGL((cg_init_kernel<T, U, decltype(e)::value>), grid, dim3(256), 0, st, *a, nseg, 2);
        return az_launch_status();
      });
    hipLaunchKernelGGL((cg_init_kernel<T, U, KR_SEG_E>), grid, dim3(256), 0, st, *a, nseg, 0);
    hipLaunchKernelGGL((cg_init_kernel<T, U, KR_SEG_E>), grid1, dim3(256), 0, st, *a, nseg, 1);
    return az_launch_status();
  });
}

int az_cg_step(const AzCgArgs* a, az_stream_t stream) {
  const int rc = check_cg(a);
  if (rc != AZ_OK) return rc;
  AZ_REQUIRE(a->Ap && a->rr && (a->out || a->p_io), AZ_E_NULL);
  AZ_REQUIRE(a->rr != a->rr_out, AZ_E_UNSUPPORTED);
  const int64_t nseg = segments(a->dim);
  dim3 grid;
  AZ_REQUIRE(grid_for(a->rows, nseg, grid), AZ_E_SHAPE);
  hipStream_t st = az_s(stream);
  return dispatch_types(a->state_dtype, a->io_dtype, [&](auto t, auto u) {
    using T = decltype(t);
    using U = decltype(u);
    if (nseg == 1)
      return dispatch_e(short_e(a->dim), [&](auto e) {
        hipLaunchKernelGGL((cg_step_short_kernel<T, U, decltype(e)::value>), grid, dim3(256), 0, st, *a);
        return az_launch_status();
      });
    hipLaunchKernelGGL((cg_step_long_kernel<T, U>), grid, dim3(256), 0, st, *a, nseg, 0);
    hipLaunchKernelGGL((cg_step_long_kernel<T, U>), grid, dim3(256), 0, st, *a, nseg, 1);
    if (!a->out) hipLaunchKernelGGL((cg_step_long_kernel<T, U>), grid, dim3(256), 0, st, *a, nseg, 2);
    return az_launch_status();
  });
}

int az_gmres_init(const AzGmresArgs* a, az_stream_t stream) {
  const int rc = check_gmres(a);
  if (rc != AZ_OK) return rc;
  AZ_REQUIRE(a->r0 && a->v_io, AZ_E_NULL);
  const int64_t nseg = segments(a->dim);
  dim3 grid;
  AZ_REQUIRE(grid_for(a->rows, nseg, grid), AZ_E_SHAPE);
  hipStream_t st = az_s(stream);
  return dispatch_types(a->state_dtype, a->io_dtype, [&](auto t, auto u) {
    using T = decltype(t);
    using U = decltype(u);
    if (nseg == 1)
      return dispatch_e(short_e(a->dim), [&](auto e) {
        hipLaunchKernelGGL((gmres_init_kernel<T, U, decltype(e)::value>), grid, dim3(256), 0, st, *a, nseg, 2);
        return az_launch_status();
      });
    hipLaunchKernelGGL((gmres_init_kernel<T, U, KR_SEG_E>), grid, dim3(256), 0, st, *a, nseg, 0);
    hipLaunchKernelGGL((gmres_init_kernel<T, U, KR_SEG_E>), grid, dim3(256), 0, st, *a, nseg, 1);
    return az_launch_status();
  });
}

int az_gmres_arnoldi(const AzGmresArgs* a, az_stream_t stream) {
  const int rc = check_gmres(a);
  if (rc != AZ_OK) return rc;
  AZ_REQUIRE(a->j >= 0 && a->j < a->iterations, AZ_E_SHAPE);
  AZ_REQUIRE(a->w && (a->j + 1 == a->iterations || a->v_io), AZ_E_NULL);
  const int64_t nseg = segments(a->dim);
  dim3 grid;
  AZ_REQUIRE(grid_for(a->rows, nseg, grid), AZ_E_SHAPE);
  hipStream_t st = az_s(stream);
  return dispatch_types(a->state_dtype, a->io_dtype, [&](auto t, auto u) {
    using T = decltype(t);
    using U = decltype(u);
    if (nseg == 1)
      return dispatch_e(short_e(a->dim), [&](auto e) {
        hipLaunchKernelGGL((gmres_arnoldi_short_kernel<T, U, decltype(e)::value>), grid, dim3(256), 0, st, *a);
        return az_launch_status();
      });
    for (int pass = 0; pass <= a->j + 1; ++pass)
      hipLaunchKernelGGL((gmres_mgs_long_kernel<T>), grid, dim3(256), 0, st, *a, nseg, pass);
    hipLaunchKernelGGL((gmres_normalize_long_kernel<T, U>), grid, dim3(256), 0, st, *a, nseg);
    return az_launch_status();
  });
}

int az_gmres_finish(const AzGmresArgs* a, az_stream_t stream) {
  const int rc = check_gmres(a);
  if (rc != AZ_OK) return rc;
  AZ_REQUIRE(a->out, AZ_E_NULL);
  const int64_t nseg = segments(a->dim);
  dim3 grid;
  AZ_REQUIRE(grid_for(a->rows, nseg, grid), AZ_E_SHAPE);
  const int64_t rblocks = (a->rows + 255) / 256;
  AZ_REQUIRE(rblocks <= (int64_t)0x7FFFFFFF, AZ_E_SHAPE);
  hipStream_t st = az_s(stream);
  return dispatch_types(a->state_dtype, a->io_dtype, [&](auto t, auto u) {
    using T = decltype(t);
    using U = decltype(u);
    hipLaunchKernelGGL((gmres_backsolve_kernel<T>), dim3((unsigned)rblocks), dim3(256), 0, st, *a);
    if (nseg == 1)
      return dispatch_e(short_e(a->dim), [&](auto e) {
        hipLaunchKernelGGL((gmres_combine_kernel<T, U, decltype(e)::value>), grid, dim3(256), 0, st, *a, nseg);
        return az_launch_status();
      });
    hipLaunchKernelGGL((gmres_combine_kernel<T, U, KR_SEG_E>), grid, dim3(256), 0, st, *a, nseg);
    return az_launch_status();
  });
}

}  // extern "C"
