// Input gradient of multi-head softmax attention (the pullback torch.autograd records behind azula/nn/attention.py:89-108,
// 112-156), fp32 on v_mfma_f32_32x32x2_f32 with fp32 accumulation.  For O = P V, P = softmax(scale Q K^T + mask):
//     Delta_t = sum_c dO_tc O_tc     dV = P^T dO     dP = dO V^T     dS = P o (dP - Delta)     dQ = scale dS K     dK = scale dS^T Q
// Eight contractions against the forward's two: Q K^T three times (statistics, dK / dV pass, dQ pass), dO V^T twice, and P^T dO,
// dS^T Q, dS K once each.  P is recomputed from the row log-sum-exp (kept in log2 units, hardware exp2); it never exists as an
// L x L tensor.  One entry, three launches:
//   (a) statistics : one wave = 32 queries, walks the key tiles with the online softmax -> lse2[t] = m + log2(l), Delta[t]
//   (b) dK, dV     : one wave = 32 keys (K, V fragments in registers), walks the query tiles (Q, dO tiles shared through LDS);
//                    S = Q K^T puts the key on the lane and 16 queries in the registers, so P and dS feed the second pair of
//                    MFMAs (dV^T += dO^T P, dK^T += Q^T dS) directly as B operands -- the forward kernel's trick, transposed
//   (c) dQ         : one wave = 32 queries (Q, dO fragments in registers), walks the key tiles (K, V tiles through LDS);
//                    S^T = K Q^T puts the query on the lane, dQ^T += K^T dS^T
// Every output element is accumulated by ONE wave in a fixed order and stored once: no atomics, no cross-workgroup sums -- two
// calls give the same bits.  A cotangent has no range: nothing here takes a half-precision form.  Masked pairs get P = 0
// exactly; a 32 x 32 tile without a live pair is skipped.  A query row without any live key is outside the contract.
#include "common.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
constexpr float kLog2e = 1.4426950408889634f;

// Row of a 32 x 32 MFMA result held in register r of a lane in half h2 (the column is lane & 31).
__device__ __forceinline__ int row_of(int r, int h2) { return (r & 3) + 8 * (r >> 2) + 4 * h2; }

template <int D>
struct Cfg {
  static constexpr int LS = D + 4;               // LDS row stride: 16-byte fragment reads without bank conflicts
  static constexpr int KJ = D / 8;               // 8 channels (4 per lane half) per group of four MFMAs
  static constexpr int DT = D >= 32 ? D / 32 : 1;  // 32-channel tiles of a [channel][token] accumulator
};

// Rows [t0, t0 + 32) of a (tokens, D) tensor with token stride `tstride` -> dst[32][LS]; rows past T are zero.
template <int D>
__device__ __forceinline__ void stage32(float* dst, const float* src, int64_t tstride, int t0, int T) {
  constexpr int LS = Cfg<D>::LS, Q4 = D / 4;
  for (int e = threadIdx.x; e < 32 * Q4; e += 256) {
    const int r = e / Q4, c4 = e % Q4;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (t0 + r < T) v = *reinterpret_cast<const float4*>(src + (int64_t)(t0 + r) * tstride + 4 * c4);
    *reinterpret_cast<float4*>(dst + r * LS + 4 * c4) = v;
  }
}

// The lane's row as the register operand of nt_tile: channels 8 jj + 4 h2 + (0..3).  row == nullptr: zeros.
template <int D>
__device__ __forceinline__ void load_frag(float (&f)[Cfg<D>::KJ][4], const float* row, int h2) {
#pragma unroll
  for (int jj = 0; jj < Cfg<D>::KJ; ++jj) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (row) v = *reinterpret_cast<const float4*>(row + 8 * jj + 4 * h2);
    f[jj][0] = v.x, f[jj][1] = v.y, f[jj][2] = v.z, f[jj][3] = v.w;
  }
}

// X[i][j] = sum_c A[i][c] B[j][c]: A = an LDS tile (row i), B = the register fragment of the lane's row j = lane & 31.
// Result: register r of the lane = X[row_of(r, h2)][lane & 31].
template <int D>
__device__ __forceinline__ f32x16 nt_tile(const float* As, const float (&bf)[Cfg<D>::KJ][4], int ql, int h2) {
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  const float* ar = As + ql * Cfg<D>::LS + 4 * h2;
#pragma unroll
  for (int jj = 0; jj < Cfg<D>::KJ; ++jj) {
    const float4 af = *reinterpret_cast<const float4*>(ar + 8 * jj);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(af.x, bf[jj][0], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(af.y, bf[jj][1], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(af.z, bf[jj][2], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(af.w, bf[jj][3], acc, 0, 0, 0);
  }
  return acc;
}

// Y[c][j] += sum_i X[i][c] W[i][j]: X = an LDS tile (row i, channel c), W = a 32 x 32 result in registers (row i in the
// registers, column j on the lane).  Tile ct of the accumulator holds the channels 32 ct + (0..31).
template <int D>
__device__ __forceinline__ void tn_acc(f32x16 (&acc)[Cfg<D>::DT], const float* Xs, const f32x16& w, int ql, int h2) {
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const float* xr = Xs + row_of(r, h2) * Cfg<D>::LS + ql;
#pragma unroll
    for (int ct = 0; ct < Cfg<D>::DT; ++ct) {
      const float xv = (D >= 32 || ql < D) ? xr[32 * ct] : 0.f;
      acc[ct] = __builtin_amdgcn_mfma_f32_32x32x2f32(xv, w[r], acc[ct], 0, 0, 0);
    }
  }
}

// The lane's row of a [channel][token] accumulator: registers 4 g .. 4 g + 3 of tile ct = channels 32 ct + 8 g + 4 h2 + (0..3).
template <int D>
__device__ __forceinline__ void store_acc(float* row, const f32x16 (&acc)[Cfg<D>::DT], float mul, int h2) {
#pragma unroll
  for (int ct = 0; ct < Cfg<D>::DT; ++ct)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int c = 32 * ct + 8 * g + 4 * h2;
      if (c < D)
        *reinterpret_cast<float4*>(row + c) =
            make_float4(acc[ct][4 * g] * mul, acc[ct][4 * g + 1] * mul, acc[ct][4 * g + 2] * mul, acc[ct][4 * g + 3] * mul);
    }
}

// (a) grid = (ceil(T / 128), heads, batch); wave w of a block owns the queries 128 bx + 32 w + (0..31).
template <int D>
__global__ __launch_bounds__(256) void attn_bwd_stats_kernel(AzAttnBwdArgs a) {
  constexpr int LS = Cfg<D>::LS, KJ = Cfg<D>::KJ;
  __shared__ __attribute__((aligned(16))) float Ks[32 * LS];
  const int T = a.tokens, b = blockIdx.z, h = blockIdx.y;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, ql = lane & 31, h2 = lane >> 5;
  const int tl = blockIdx.x * 128 + 32 * w + ql;
  const bool qok = tl < T;
  float qf[KJ][4];
  load_frag<D>(qf, qok ? a.q + (int64_t)b * a.q_bstride + (int64_t)h * a.q_hstride + (int64_t)tl * a.q_tstride : nullptr, h2);
  const float* kb = a.k + (int64_t)b * a.k_bstride + (int64_t)h * a.k_hstride;
  const uint8_t* mrow = a.mask ? a.mask + (int64_t)b * a.mask_bstride + (int64_t)h * a.mask_hstride + (int64_t)tl * T : nullptr;
  const float sl2 = a.scale * kLog2e;
  float m = -INFINITY, l = 0.f;  // running maximum (shared by the two lane halves of a query) and this half's share of the sum
  for (int k0 = 0; k0 < T; k0 += 32) {
    __syncthreads();
    stage32<D>(Ks, kb, a.k_tstride, k0, T);
    __syncthreads();
    unsigned live = 0;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int key = k0 + row_of(r, h2);
      const bool ok = qok && key < T && (mrow == nullptr || mrow[key] != 0);
      live |= (unsigned)ok << r;
    }
    if (__ballot(live != 0) == 0) continue;  // (wave-uniform; the barriers sit at the loop head)
    f32x16 s = nt_tile<D>(Ks, qf, ql, h2);
    float tmax = -INFINITY;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      s[r] = ((live >> r) & 1u) ? s[r] * sl2 : -INFINITY;
      tmax = fmaxf(tmax, s[r]);
    }
    tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
    const float mn = fmaxf(m, tmax);
    if (mn > -INFINITY) {
      float sum = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) sum += __builtin_amdgcn_exp2f(s[r] - mn);
      l = l * __builtin_amdgcn_exp2f(m - mn) + sum;
      m = mn;
    }
  }
  l += __shfl_xor(l, 32, 64);
  float dl = 0.f;
  if (qok) {
    float of[KJ][4], gf[KJ][4];
    load_frag<D>(of, a.out + (int64_t)b * a.o_bstride + (int64_t)h * a.o_hstride + (int64_t)tl * a.o_tstride, h2);
    load_frag<D>(gf, a.dout + (int64_t)b * a.do_bstride + (int64_t)h * a.do_hstride + (int64_t)tl * a.do_tstride, h2);
#pragma unroll
    for (int jj = 0; jj < KJ; ++jj)
#pragma unroll
      for (int i = 0; i < 4; ++i) dl += of[jj][i] * gf[jj][i];
  }
  dl += __shfl_xor(dl, 32, 64);
  if (qok && h2 == 0) {
    const int64_t bh = ((int64_t)b * a.heads + h) * T + tl;
    a.workspace[bh] = m + __builtin_amdgcn_logf(l);  // (v_log_f32: base 2)
    a.workspace[(int64_t)a.batch * a.heads * T + bh] = dl;
  }
}

// (b) grid = (ceil(T / 128), heads, batch); wave w of a block owns the keys 128 bx + 32 w + (0..31).
template <int D>
__global__ __launch_bounds__(256) void attn_bwd_dkdv_kernel(AzAttnBwdArgs a) {
  constexpr int LS = Cfg<D>::LS, KJ = Cfg<D>::KJ, DT = Cfg<D>::DT;
  __shared__ __attribute__((aligned(16))) float Qs[32 * LS];
  __shared__ __attribute__((aligned(16))) float Gs[32 * LS];
  __shared__ float st[64];  // [0, 32): lse2, [32, 64): Delta of the query tile
  const int T = a.tokens, b = blockIdx.z, h = blockIdx.y;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, ql = lane & 31, h2 = lane >> 5;
  const int sl = blockIdx.x * 128 + 32 * w + ql;
  const bool kok = sl < T;
  float kf[KJ][4], vf[KJ][4];
  load_frag<D>(kf, kok ? a.k + (int64_t)b * a.k_bstride + (int64_t)h * a.k_hstride + (int64_t)sl * a.k_tstride : nullptr, h2);
  load_frag<D>(vf, kok ? a.v + (int64_t)b * a.v_bstride + (int64_t)h * a.v_hstride + (int64_t)sl * a.v_tstride : nullptr, h2);
  const float* qb = a.q + (int64_t)b * a.q_bstride + (int64_t)h * a.q_hstride;
  const float* gb = a.dout + (int64_t)b * a.do_bstride + (int64_t)h * a.do_hstride;
  const float* lse = a.workspace + ((int64_t)b * a.heads + h) * T;
  const float* dlt = lse + (int64_t)a.batch * a.heads * T;
  const uint8_t* mb = a.mask ? a.mask + (int64_t)b * a.mask_bstride + (int64_t)h * a.mask_hstride : nullptr;
  const float sl2 = a.scale * kLog2e;
  f32x16 dk[DT], dv[DT];
#pragma unroll
  for (int ct = 0; ct < DT; ++ct)
#pragma unroll
    for (int r = 0; r < 16; ++r) dk[ct][r] = 0.f, dv[ct][r] = 0.f;
  for (int q0 = 0; q0 < T; q0 += 32) {
    __syncthreads();
    stage32<D>(Qs, qb, a.q_tstride, q0, T);
    stage32<D>(Gs, gb, a.do_tstride, q0, T);
    if (threadIdx.x < 64) {
      const int t = q0 + (threadIdx.x & 31);
      st[threadIdx.x] = t < T ? (threadIdx.x < 32 ? lse[t] : dlt[t]) : 0.f;
    }
    __syncthreads();
    unsigned live = 0;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int t = q0 + row_of(r, h2);
      const bool ok = kok && t < T && (mb == nullptr || mb[(int64_t)t * T + sl] != 0);
      live |= (unsigned)ok << r;
    }
    if (__ballot(live != 0) == 0) continue;
    f32x16 s = nt_tile<D>(Qs, kf, ql, h2);   // S[t][s]
    f32x16 dp = nt_tile<D>(Gs, vf, ql, h2);  // dP[t][s]
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int tr = row_of(r, h2);
      const float p = ((live >> r) & 1u) ? __builtin_amdgcn_exp2f(__builtin_fmaf(s[r], sl2, -st[tr])) : 0.f;
      s[r] = p;
      dp[r] = p * (dp[r] - st[32 + tr]);
    }
    tn_acc<D>(dv, Gs, s, ql, h2);   // dV^T[c][s] += sum_t dO[t][c] P[t][s]
    tn_acc<D>(dk, Qs, dp, ql, h2);  // dK^T[c][s] += sum_t Q[t][c] dS[t][s]
  }
  if (kok) {
    store_acc<D>(a.dv + (int64_t)b * a.dv_bstride + (int64_t)h * a.dv_hstride + (int64_t)sl * a.dv_tstride, dv, 1.f, h2);
    store_acc<D>(a.dk + (int64_t)b * a.dk_bstride + (int64_t)h * a.dk_hstride + (int64_t)sl * a.dk_tstride, dk, a.scale, h2);
  }
}

// (c) grid = (ceil(T / 128), heads, batch); wave w of a block owns the queries 128 bx + 32 w + (0..31).
template <int D>
__global__ __launch_bounds__(256) void attn_bwd_dq_kernel(AzAttnBwdArgs a) {
  constexpr int LS = Cfg<D>::LS, KJ = Cfg<D>::KJ, DT = Cfg<D>::DT;
  __shared__ __attribute__((aligned(16))) float Ks[32 * LS];
  __shared__ __attribute__((aligned(16))) float Vs[32 * LS];
  const int T = a.tokens, b = blockIdx.z, h = blockIdx.y;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, ql = lane & 31, h2 = lane >> 5;
  const int tl = blockIdx.x * 128 + 32 * w + ql;
  const bool qok = tl < T;
  float qf[KJ][4], gf[KJ][4];
  load_frag<D>(qf, qok ? a.q + (int64_t)b * a.q_bstride + (int64_t)h * a.q_hstride + (int64_t)tl * a.q_tstride : nullptr, h2);
  load_frag<D>(gf, qok ? a.dout + (int64_t)b * a.do_bstride + (int64_t)h * a.do_hstride + (int64_t)tl * a.do_tstride : nullptr, h2);
  const float* kb = a.k + (int64_t)b * a.k_bstride + (int64_t)h * a.k_hstride;
  const float* vb = a.v + (int64_t)b * a.v_bstride + (int64_t)h * a.v_hstride;
  const int64_t bh = ((int64_t)b * a.heads + h) * T + tl;
  const float lse = qok ? a.workspace[bh] : 0.f;
  const float dlt = qok ? a.workspace[(int64_t)a.batch * a.heads * T + bh] : 0.f;
  const uint8_t* mrow = a.mask ? a.mask + (int64_t)b * a.mask_bstride + (int64_t)h * a.mask_hstride + (int64_t)tl * T : nullptr;
  const float sl2 = a.scale * kLog2e;
  f32x16 dq[DT];
#pragma unroll
  for (int ct = 0; ct < DT; ++ct)
#pragma unroll
    for (int r = 0; r < 16; ++r) dq[ct][r] = 0.f;
  for (int k0 = 0; k0 < T; k0 += 32) {
    __syncthreads();
    stage32<D>(Ks, kb, a.k_tstride, k0, T);
    stage32<D>(Vs, vb, a.v_tstride, k0, T);
    __syncthreads();
    unsigned live = 0;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int key = k0 + row_of(r, h2);
      const bool ok = qok && key < T && (mrow == nullptr || mrow[key] != 0);
      live |= (unsigned)ok << r;
    }
    if (__ballot(live != 0) == 0) continue;
    f32x16 s = nt_tile<D>(Ks, qf, ql, h2);   // S^T[s][t]
    f32x16 dp = nt_tile<D>(Vs, gf, ql, h2);  // dP^T[s][t]
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float p = ((live >> r) & 1u) ? __builtin_amdgcn_exp2f(__builtin_fmaf(s[r], sl2, -lse)) : 0.f;
      dp[r] = p * (dp[r] - dlt);
    }
    tn_acc<D>(dq, Ks, dp, ql, h2);  // dQ^T[c][t] += sum_s K[s][c] dS^T[s][t]
  }
  if (qok) store_acc<D>(a.dq + (int64_t)b * a.dq_bstride + (int64_t)h * a.dq_hstride + (int64_t)tl * a.dq_tstride, dq, a.scale, h2);
}

template <int D>
int attn_bwd_launch(const AzAttnBwdArgs* a, hipStream_t s) {
  const dim3 grid((unsigned)((a->tokens + 127) / 128), (unsigned)a->heads, (unsigned)a->batch);
  hipLaunchKernelGGL(attn_bwd_stats_kernel<D>, grid, dim3(256), 0, s, *a);
  hipLaunchKernelGGL(attn_bwd_dkdv_kernel<D>, grid, dim3(256), 0, s, *a);
  hipLaunchKernelGGL(attn_bwd_dq_kernel<D>, grid, dim3(256), 0, s, *a);
  return az_launch_status();
}

// ------------------------------------------------------------------------------------------------------------------------
// q / k preparation outside the attention kernel (forward-keep side) and its pullback.  One (token, head, q | k) row is held by
// D / 4 adjacent lanes, four channels each: the row sums are butterflies inside that lane group.  HBM-bound: 8 B / element forward,
// 12 B / element backward (+ the tables).
struct QkPrepArgs {
  const float* x[2];  // raw q, k
  const float* g[2];  // backward: cotangents of q^, k^
  float* y[2];        // forward: q^, k^; backward: cotangents of q, k
  int64_t xb, xt, xh, gb, gt, gh, yb, yt, yh;
  int64_t rows;  // batch * tokens * heads * 2
  int T, H, rms;
  float inv_n, eps;
  const float* cs;
  const float* sn;
  const float* w[2];  // learned gains of q, k (D floats each) between the RMS norm and the rotation, or null
};

template <int G>
__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
  for (int o = G / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// GAIN: q^ = rope(w rms_norm(q)); backward u = R^T g, qg = w u, dx = r (qg - xh mean(qg xh)).  Without it the instantiation is
// the kernel as it was, bit for bit.
template <int D, bool BWD, bool GAIN>
__global__ __launch_bounds__(256) void qk_prep_kernel(QkPrepArgs p) {
  constexpr int G = D / 4, RPB = 256 / G;
  const int gl = threadIdx.x % G;
  const int64_t stride = (int64_t)gridDim.x * RPB;
  const int64_t iters = (p.rows + stride - 1) / stride;
  for (int64_t it = 0; it < iters; ++it) {  // (the same trip count for every lane: the butterflies run converged)
    const int64_t row = (it * gridDim.x + blockIdx.x) * RPB + threadIdx.x / G;
    const bool valid = row < p.rows;
    const int which = (int)(row & 1);
    const int hh = (int)((row >> 1) % p.H);
    const int t = (int)(((row >> 1) / p.H) % p.T);
    const int64_t b = (row >> 1) / ((int64_t)p.H * p.T);
    float4 x = make_float4(0.f, 0.f, 0.f, 0.f), g = x;
    if (valid) {
      x = *reinterpret_cast<const float4*>(p.x[which] + b * p.xb + (int64_t)t * p.xt + (int64_t)hh * p.xh + 4 * gl);
      if (BWD) g = *reinterpret_cast<const float4*>(p.g[which] + b * p.gb + (int64_t)t * p.gt + (int64_t)hh * p.gh + 4 * gl);
    }
    float c0 = 1.f, s0 = 0.f, c1 = 1.f, s1 = 0.f;
    if (p.cs != nullptr && valid) {
      const int64_t o = ((int64_t)t * p.H + hh) * (D / 2) + 2 * gl;
      c0 = p.cs[o], c1 = p.cs[o + 1], s0 = p.sn[o], s1 = p.sn[o + 1];
    }
    float r = 1.f;
    if (p.rms) r = rsqrtf(group_sum<G>(x.x * x.x + x.y * x.y + x.z * x.z + x.w * x.w) * p.inv_n + p.eps);
    float4 w = make_float4(1.f, 1.f, 1.f, 1.f);
    if (GAIN) {
      const float* wp = p.w[which];  // (rows alternate q / k: the pointer, not the branch, differs between lane groups)
      if (wp != nullptr) w = *reinterpret_cast<const float4*>(wp + 4 * gl);
    }
    float4 y;
    if (!BWD) {
      x.x *= r, x.y *= r, x.z *= r, x.w *= r;
      if (GAIN) x.x *= w.x, x.y *= w.y, x.z *= w.z, x.w *= w.w;
      y = make_float4(x.x * c0 - x.y * s0, x.x * s0 + x.y * c0, x.z * c1 - x.w * s1, x.z * s1 + x.w * c1);
    } else {
      // the rotation's transpose (pairs turned by -theta), then the RMS-norm pullback dx = r (g - xh mean(g xh))
      float4 u = make_float4(g.x * c0 + g.y * s0, g.y * c0 - g.x * s0, g.z * c1 + g.w * s1, g.w * c1 - g.z * s1);
      if (GAIN) u.x *= w.x, u.y *= w.y, u.z *= w.z, u.w *= w.w;
      y = u;
      if (p.rms) {
        const float4 xh = make_float4(x.x * r, x.y * r, x.z * r, x.w * r);
        const float mq = group_sum<G>(u.x * xh.x + u.y * xh.y + u.z * xh.z + u.w * xh.w) * p.inv_n;
        y = make_float4(r * (u.x - xh.x * mq), r * (u.y - xh.y * mq), r * (u.z - xh.z * mq), r * (u.w - xh.w * mq));
      }
    }
    if (valid) *reinterpret_cast<float4*>(p.y[which] + b * p.yb + (int64_t)t * p.yt + (int64_t)hh * p.yh + 4 * gl) = y;
  }
}

template <bool BWD, bool GAIN>
int qk_prep_launch(const QkPrepArgs& p, int head_dim, hipStream_t s) {
  const int rpb = 256 / (head_dim / 4);
  const dim3 grid((unsigned)az_stream_grid(p.rows, rpb));
  switch (head_dim) {
    case 16: hipLaunchKernelGGL((qk_prep_kernel<16, BWD, GAIN>), grid, dim3(256), 0, s, p); break;
    case 32: hipLaunchKernelGGL((qk_prep_kernel<32, BWD, GAIN>), grid, dim3(256), 0, s, p); break;
    case 64: hipLaunchKernelGGL((qk_prep_kernel<64, BWD, GAIN>), grid, dim3(256), 0, s, p); break;
    default: hipLaunchKernelGGL((qk_prep_kernel<128, BWD, GAIN>), grid, dim3(256), 0, s, p); break;
  }
  return az_launch_status();
}

inline bool head_dim_ok(int d) { return d == 16 || d == 32 || d == 64 || d == 128; }

}  // namespace

extern "C" {

int az_attention_bwd_f32(const AzAttnBwdArgs* a, az_stream_t stream) {
  AZ_REQUIRE(a && a->q && a->k && a->v && a->out && a->dout && a->dq && a->dk && a->dv && a->workspace, AZ_E_NULL);
  AZ_REQUIRE(a->batch > 0 && a->batch < 65536 && a->heads > 0 && a->heads < 65536 && a->tokens > 0, AZ_E_SHAPE);
  AZ_REQUIRE(head_dim_ok(a->head_dim), AZ_E_UNSUPPORTED);
  AZ_REQUIRE(AZ_ALIGNED16(a->q) && AZ_ALIGNED16(a->k) && AZ_ALIGNED16(a->v) && AZ_ALIGNED16(a->out) && AZ_ALIGNED16(a->dout) &&
                 AZ_ALIGNED16(a->dq) && AZ_ALIGNED16(a->dk) && AZ_ALIGNED16(a->dv) && AZ_ALIGNED16(a->workspace),
             AZ_E_ALIGN);
  const int64_t strides[] = {a->q_bstride,  a->q_tstride,  a->q_hstride,  a->k_bstride,  a->k_tstride,  a->k_hstride,
                             a->v_bstride,  a->v_tstride,  a->v_hstride,  a->o_bstride,  a->o_tstride,  a->o_hstride,
                             a->do_bstride, a->do_tstride, a->do_hstride, a->dq_bstride, a->dq_tstride, a->dq_hstride,
                             a->dk_bstride, a->dk_tstride, a->dk_hstride, a->dv_bstride, a->dv_tstride, a->dv_hstride};
  for (int64_t s : strides) AZ_REQUIRE(s % 4 == 0, AZ_E_ALIGN);
  switch (a->head_dim) {
    case 16: return attn_bwd_launch<16>(a, az_s(stream));
    case 32: return attn_bwd_launch<32>(a, az_s(stream));
    case 64: return attn_bwd_launch<64>(a, az_s(stream));
    default: return attn_bwd_launch<128>(a, az_s(stream));
  }
}

int az_qk_prep_f32(float* q_hat, float* k_hat, const float* q, const float* k, int64_t batch, int64_t tokens, int32_t heads,
                   int32_t head_dim, int64_t in_bstride, int64_t in_tstride, int64_t in_hstride, int64_t out_bstride,
                   int64_t out_tstride, int64_t out_hstride, int32_t qk_rmsnorm, int32_t norm_dim, float eps, const float* rope_cos,
                   const float* rope_sin, az_stream_t stream) {
  return az_qk_prep_w_f32(q_hat, k_hat, q, k, batch, tokens, heads, head_dim, in_bstride, in_tstride, in_hstride, out_bstride,
                          out_tstride, out_hstride, qk_rmsnorm, norm_dim, eps, rope_cos, rope_sin, nullptr, nullptr, stream);
}

int az_qk_prep_bwd_f32(float* dq, float* dk, const float* dq_hat, const float* dk_hat, const float* q, const float* k, int64_t batch,
                       int64_t tokens, int32_t heads, int32_t head_dim, int64_t g_bstride, int64_t g_tstride, int64_t g_hstride,
                       int64_t in_bstride, int64_t in_tstride, int64_t in_hstride, int64_t out_bstride, int64_t out_tstride,
                       int64_t out_hstride, int32_t qk_rmsnorm, int32_t norm_dim, float eps, const float* rope_cos,
                       const float* rope_sin, az_stream_t stream) {
  return az_qk_prep_bwd_w_f32(dq, dk, dq_hat, dk_hat, q, k, batch, tokens, heads, head_dim, g_bstride, g_tstride, g_hstride, in_bstride,
                              in_tstride, in_hstride, out_bstride, out_tstride, out_hstride, qk_rmsnorm, norm_dim, eps, rope_cos,
                              rope_sin, nullptr, nullptr, stream);
}

// The gains are head_dim floats each and may be null one by one (a null one is a gain of 1); with both null the launch is the
// gain-free instantiation, so the entries above keep their bits.
int az_qk_prep_w_f32(float* q_hat, float* k_hat, const float* q, const float* k, int64_t batch, int64_t tokens, int32_t heads,
                     int32_t head_dim, int64_t in_bstride, int64_t in_tstride, int64_t in_hstride, int64_t out_bstride,
                   int64_t out_tstride, int64_t out_hstride, int32_t qk_rmsnorm, int32_t norm_dim, float eps, const float* rope_cos,
                   const float* rope_sin, const float* q_weight, const float* k_weight, az_stream_t stream) {
  AZ_REQUIRE(q_hat && k_hat && q && k && (rope_cos == nullptr) == (rope_sin == nullptr), AZ_E_NULL);
  AZ_REQUIRE(batch > 0 && tokens > 0 && tokens < (1ll << 31) && heads > 0 && norm_dim >= 0 && norm_dim <= head_dim, AZ_E_SHAPE);
  AZ_REQUIRE(head_dim_ok(head_dim), AZ_E_UNSUPPORTED);
  AZ_REQUIRE(AZ_ALIGNED16(q_hat) && AZ_ALIGNED16(k_hat) && AZ_ALIGNED16(q) && AZ_ALIGNED16(k), AZ_E_ALIGN);
  const int64_t strides[] = {in_bstride, in_tstride, in_hstride, out_bstride, out_tstride, out_hstride};
  for (int64_t s : strides) AZ_REQUIRE(s % 4 == 0, AZ_E_ALIGN);
  QkPrepArgs p = {};
  p.x[0] = q, p.x[1] = k, p.y[0] = q_hat, p.y[1] = k_hat;
  p.xb = in_bstride, p.xt = in_tstride, p.xh = in_hstride, p.yb = out_bstride, p.yt = out_tstride, p.yh = out_hstride;
  p.rows = batch * tokens * heads * 2;
  p.T = (int)tokens, p.H = heads, p.rms = qk_rmsnorm != 0;
  p.inv_n = 1.0f / (float)(norm_dim ? norm_dim : head_dim), p.eps = eps;
  p.cs = rope_cos, p.sn = rope_sin;
  if (q_weight == nullptr && k_weight == nullptr) return qk_prep_launch<false, false>(p, head_dim, az_s(stream));
  AZ_REQUIRE(AZ_ALIGNED16(q_weight) && AZ_ALIGNED16(k_weight), AZ_E_ALIGN);
  p.w[0] = q_weight, p.w[1] = k_weight;
  return qk_prep_launch<false, true>(p, head_dim, az_s(stream));
}

int az_qk_prep_bwd_w_f32(float* dq, float* dk, const float* dq_hat, const float* dk_hat, const float* q, const float* k, int64_t batch,
                       int64_t tokens, int32_t heads, int32_t head_dim, int64_t g_bstride, int64_t g_tstride, int64_t g_hstride,
                       int64_t in_bstride, int64_t in_tstride, int64_t in_hstride, int64_t out_bstride, int64_t out_tstride,
                       int64_t out_hstride, int32_t qk_rmsnorm, int32_t norm_dim, float eps, const float* rope_cos,
                       const float* rope_sin, const float* q_weight, const float* k_weight, az_stream_t stream) {
  AZ_REQUIRE(dq && dk && dq_hat && dk_hat && q && k && (rope_cos == nullptr) == (rope_sin == nullptr), AZ_E_NULL);
  AZ_REQUIRE(batch > 0 && tokens > 0 && tokens < (1ll << 31) && heads > 0 && norm_dim >= 0 && norm_dim <= head_dim, AZ_E_SHAPE);
  AZ_REQUIRE(head_dim_ok(head_dim), AZ_E_UNSUPPORTED);
  AZ_REQUIRE(AZ_ALIGNED16(dq) && AZ_ALIGNED16(dk) && AZ_ALIGNED16(dq_hat) && AZ_ALIGNED16(dk_hat) && AZ_ALIGNED16(q) && AZ_ALIGNED16(k),
             AZ_E_ALIGN);
  const int64_t strides[] = {g_bstride, g_tstride, g_hstride, in_bstride, in_tstride, in_hstride, out_bstride, out_tstride, out_hstride};
  for (int64_t s : strides) AZ_REQUIRE(s % 4 == 0, AZ_E_ALIGN);
  QkPrepArgs p = {};
  p.x[0] = q, p.x[1] = k, p.g[0] = dq_hat, p.g[1] = dk_hat, p.y[0] = dq, p.y[1] = dk;
  p.xb = in_bstride, p.xt = in_tstride, p.xh = in_hstride, p.gb = g_bstride, p.gt = g_tstride, p.gh = g_hstride;
  p.yb = out_bstride, p.yt = out_tstride, p.yh = out_hstride;
  p.rows = batch * tokens * heads * 2;
  p.T = (int)tokens, p.H = heads, p.rms = qk_rmsnorm != 0;
  p.inv_n = 1.0f / (float)(norm_dim ? norm_dim : head_dim), p.eps = eps;
  p.cs = rope_cos, p.sn = rope_sin;
  if (q_weight == nullptr && k_weight == nullptr) return qk_prep_launch<true, false>(p, head_dim, az_s(stream));
  AZ_REQUIRE(AZ_ALIGNED16(q_weight) && AZ_ALIGNED16(k_weight), AZ_E_ALIGN);
  p.w[0] = q_weight, p.w[1] = k_weight;
  return qk_prep_launch<true, true>(p, head_dim, az_s(stream));
}

}  // extern "C"
