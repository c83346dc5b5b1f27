// Measurement operators of the guidance methods (azula_amd/guidance/operators.py): pixel mask, average-pool downsampling with
// its adjoint / pseudo-inverse, a separable blur, a general 2-D PSF, decimation with its adjoint, and a per-pixel channel mix.
// Planar fp32 (B, C, H, W) tensors seen as planes = B * C images of H x W.
//
//   az_op_mul_f32          y[i] = x[i] * m[i mod m_n]                                   8 B / element (+ m, cache resident)
//   az_op_avgpool_f32      y[n, i, j] = (sum_{a, b} x[n, i fh + a, j fw + b]) / (fh fw)  4 + 4 / (fh fw) B / input element
//   az_op_avgpool_adj_f32  dx[n, Y, X] = scale * g[n, Y / fh, X / fw]                    4 + 4 / (fh fw) B / output element
//   az_op_blur_f32         y = taps_h (x) taps_w correlated with x, zero or wrapped edge 8 B / element from HBM (halo: L2)
//   az_op_psf_f32          y = a general kh x kw PSF correlated with x, one PSF per plane 8 B / element; 2 kh kw FLOP / element
//   az_op_decimate_f32     y[n, i, j] = x[n, i fh + oh, j fw + ow]                       4 + 4 / (fh fw) B / input element
//   az_op_decimate_adj_f32 dx = g zero-stuffed onto the (H, W) grid                      4 + 4 / (fh fw) B / output element
//   az_op_chanmix_f32      y[b, o, p] = sum_c M[o, c] x[b, c, p]                         4 (Cin + Cout) B / pixel
//
// No atomics and a fixed summation order everywhere: two launches on the same data give the same bits.  Every index that reaches a
// pointer is an int64; work items (float4 groups, pixels, blur tiles) are a linear int64 range walked with a grid stride, so the
// plane count never sits on grid.y / grid.z.
#include "common.h"

namespace {

// ---------------------------------------------------------------------------------------------------------------- mask
// V4: m_n % 4 == 0, so a float4 of x never straddles the end of m and m is read 16 bytes at a time.  Otherwise the four factors
// are gathered one by one.  y may be x: an element is read and written by the same thread only.
template <bool V4>
__global__ __launch_bounds__(256) void op_mul_kernel(float* y, const float* x, const float* __restrict__ m, int64_t n,
                                                     int64_t m_n) {
  const int64_t n4 = n / 4;
  const bool whole = m_n == n;  // (no modulo for a full-size mask)
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t e = 4 * i;
    const float4 xv = *reinterpret_cast<const float4*>(x + e);
    float4 mv;
    if (V4) {
      mv = *reinterpret_cast<const float4*>(m + (whole ? e : e % m_n));
    } else {
      int64_t k = whole ? e : e % m_n;
      mv.x = m[k];
      k = k + 1 == m_n ? 0 : k + 1;
      mv.y = m[k];
      k = k + 1 == m_n ? 0 : k + 1;
      mv.z = m[k];
      k = k + 1 == m_n ? 0 : k + 1;
      mv.w = m[k];
    }
    *reinterpret_cast<float4*>(y + e) = make_float4(az_mul(xv.x, mv.x), az_mul(xv.y, mv.y), az_mul(xv.z, mv.z), az_mul(xv.w, mv.w));
  }
  if (blockIdx.x == 0) {  // scalar tail (n not a multiple of 4)
    for (int64_t e = n4 * 4 + threadIdx.x; e < n; e += blockDim.x) y[e] = az_mul(x[e], m[whole ? e : e % m_n]);
  }
}

// ------------------------------------------------------------------------------------------------------------- pooling
// One thread per output pixel, adjacent lanes on adjacent j: the 64 windows of a wave cover 64 * fw consecutive floats of each
// of their fh input rows.  Sum over a, then b, ascending, then one multiplication by 1 / (fh fw).
__global__ __launch_bounds__(256) void op_avgpool_kernel(float* __restrict__ y, const float* __restrict__ x, int64_t total,
                                                         int64_t Ho, int64_t Wo, int64_t W, int fh, int fw, float inv) {
  for (int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; o < total; o += (int64_t)gridDim.x * blockDim.x) {
    const int64_t j = o % Wo, ni = o / Wo;  // ni = n * Ho + i, and input row n * H + i * fh = ni * fh
    const float* src = x + (ni * fh) * W + j * fw;
    float acc = 0.f;
    for (int a = 0; a < fh; ++a)
      for (int b = 0; b < fw; ++b) acc = az_add(acc, src[(int64_t)a * W + b]);
    y[o] = az_mul(acc, inv);
  }
}

// One thread per pixel of the large grid; the fw lanes of a window read the same float of g.
__global__ __launch_bounds__(256) void op_avgpool_adj_kernel(float* __restrict__ dx, const float* __restrict__ g, int64_t total,
                                                             int64_t H, int64_t W, int64_t Wo, int fh, int fw, float scale) {
  for (int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; o < total; o += (int64_t)gridDim.x * blockDim.x) {
    const int64_t X = o % W, nY = o / W;  // nY = n * H + Y
    const int64_t Y = nY % H, n = nY / H;
    dx[o] = az_mul(scale, g[(n * (H / fh) + Y / fh) * Wo + X / fw]);
  }
}

// ---------------------------------------------------------------------------------------------------------------- blur
// A workgroup of 4 waves owns an output tile of th x 64 pixels of one plane (th: blur_tile_rows, at most 32).
//   1. stage   S[r][c] = x~[i0 + r - rh][j0 + c - rw]   r < rows + nh - 1, c < cols + nw - 1   (rows, cols: the part of the tile
//                                                                                               inside the image)
//   2. row     R[r][j] = sum_b taps_w[b] S[r][j + b]     r < rows + nh - 1, j < cols
//   3. column  y[i0 + i][j0 + j] = sum_a taps_h[a] R[i + a][j]
// Every sum is one chain of fused multiply-adds from 0, taps ascending.  A wave takes whole rows and its lanes consecutive
// columns, so the staging loads and the stores are contiguous runs of a row, and every LDS access of all three phases is 64
// consecutive words: no two lanes of a wave ever share a bank, whatever the row stride, so the rows carry no padding.  The tap
// index is the same in every lane: the taps are read through the scalar cache, not from LDS.
constexpr int BLUR_TW = 64, BLUR_TH_MAX = 32, BLUR_MAX_TAPS = 65;
constexpr int BLUR_LDS_BIG = 16384, BLUR_LDS_SMALL = 6144;  // floats: 64 KiB (two workgroups per CU) / 24 KiB (six)

// floats of LDS a tile of th rows needs: S is (th + nh - 1) x (64 + nw - 1), R is (th + nh - 1) x 64
inline int blur_lds_floats(int th, int nh, int nw) { return (th + nh - 1) * (BLUR_TW + nw - 1 + BLUR_TW); }

// the tallest tile (a multiple of 4 rows, at most 32) that fits 64 KiB; 20 rows at 65 x 65 taps
inline int blur_tile_rows(int nh, int nw) {
  int th = BLUR_LDS_BIG / (BLUR_TW + nw - 1 + BLUR_TW) - (nh - 1);
  th = th > BLUR_TH_MAX ? BLUR_TH_MAX : th;
  return th & ~3;
}

template <int LDS_FLOATS, bool CIRCULAR>
__global__ __launch_bounds__(256) void op_blur_kernel(float* __restrict__ y, const float* __restrict__ x,
                                                      const float* __restrict__ taps_h, int nh, const float* __restrict__ taps_w,
                                                      int nw, int64_t H, int64_t W, int th, int64_t tiles_y, int64_t tiles_x,
                                                      int64_t total) {
  __shared__ float lds[LDS_FLOATS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int rh = nh / 2, rw = nw / 2;
  const int sw = BLUR_TW + nw - 1;  // row stride of S
  float* S = lds;
  float* R = lds + (th + nh - 1) * sw;
  for (int64_t t = blockIdx.x; t < total; t += gridDim.x) {
    const int64_t tx = t % tiles_x, q = t / tiles_x;
    const int64_t ty = q % tiles_y, plane = q / tiles_y;
    const int64_t i0 = ty * th, j0 = tx * BLUR_TW;
    const int rows = (int)(H - i0 < th ? H - i0 : th), cols = (int)(W - j0 < BLUR_TW ? W - j0 : BLUR_TW);
    const int srows = rows + nh - 1, scols = cols + nw - 1;
    const float* xp = x + plane * H * W;
    // 1. stage.  i0 + r - rh lies in (-H, 2 H) and j0 + c - rw in (-W, 2 W) (circular: rh < H, rw < W), so one wrap suffices.
    for (int r = wave; r < srows; r += 4) {
      int64_t gy = i0 + r - rh;
      bool row_in = true;
      if (CIRCULAR) gy = gy < 0 ? gy + H : (gy >= H ? gy - H : gy);
      else row_in = gy >= 0 && gy < H;
      for (int c = lane; c < scols; c += 64) {
        int64_t gx = j0 + c - rw;
        bool in = row_in;
        if (CIRCULAR) gx = gx < 0 ? gx + W : (gx >= W ? gx - W : gx);
        else in = in && gx >= 0 && gx < W;
        S[r * sw + c] = in ? xp[gy * W + gx] : 0.f;
      }
    }
    __syncthreads();
    // 2. row pass.  A wave owns the rows wave, wave + 4, ... and runs four of them at a time: four independent chains behind one
    // scalar tap, so a chain's LDS and FMA latency is covered by the other three (a row past the end re-reads the last row and
    // is not written).
    if (lane < cols) {
      for (int r0 = wave; r0 < srows; r0 += 16) {
        const float* s[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) s[k] = S + (r0 + 4 * k < srows ? r0 + 4 * k : srows - 1) * sw + lane;
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
        for (int b = 0; b < nw; ++b) {
          const float t = taps_w[b];
#pragma unroll
          for (int k = 0; k < 4; ++k) acc[k] = __builtin_fmaf(t, s[k][b], acc[k]);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (r0 + 4 * k < srows) R[(r0 + 4 * k) * BLUR_TW + lane] = acc[k];
      }
    }
    __syncthreads();
    // 3. column pass, the same way over the output rows
    if (lane < cols) {
      for (int r0 = wave; r0 < rows; r0 += 16) {
        const float* s[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) s[k] = R + (r0 + 4 * k < rows ? r0 + 4 * k : rows - 1) * BLUR_TW + lane;
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
        for (int a = 0; a < nh; ++a) {
          const float t = taps_h[a];
#pragma unroll
          for (int k = 0; k < 4; ++k) acc[k] = __builtin_fmaf(t, s[k][a * BLUR_TW], acc[k]);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (r0 + 4 * k < rows) y[(plane * H + i0 + r0 + 4 * k) * W + j0 + lane] = acc[k];
      }
    }
    __syncthreads();  // (the next tile of this workgroup overwrites S and R)
  }
}

// ----------------------------------------------------------------------------------------------------------------- PSF
// A general (non-separable) kh x kw correlation, shaped as the blur: a workgroup of 4 waves owns a 16 x 64 output tile of one
// plane and stages S[r][c] = x~[i0 + r - rh][j0 + c - rw], r < rows + kh - 1, c < cols + kw - 1.  A wave takes blocks of R
// consecutive output rows and its lanes consecutive columns, so every LDS access is 64 consecutive words.  A thread carries the
// R outputs (i0 + k, j), k < R, of its block in registers and walks the staged rows r of the block top down: the value
// S[r][j + b] is read ONCE and feeds the R chains acc[k] += psf[r - k][b] * S[r][j + b] -- one LDS read per R fused
// multiply-adds (R + kh - 1 staged rows for R kh tap rows) where the blur's form pays one per multiply-add.  For every output
// the tap row a = r - k ascends with r and b ascends inside a row: the documented order, whatever R.  The first and last R - 1
// staged rows of a block reach only some of the outputs; which ones is known at compile time (kh >= R), so those rows are
// unrolled with exactly their chains and nothing is predicated.  The taps are uniform in a workgroup and come through the
// scalar cache.  R = 4 from kh = 5 on, 2 for 3, 1 for 1: each wave of a full tile has one block.  (32 rows with R = 8 halve the
// LDS reads again but leave half as many workgroups: 237 us against 182 us on 4 x 3 x 256 x 256 at 61 x 61, where 384 tiles of 32
// rows do not fill 256 CUs.)
constexpr int PSF_TW = 64, PSF_TH = 16, PSF_MAX = 65;
constexpr int PSF_LDS_BIG = 10240, PSF_LDS_SMALL = 4096;  // floats: 40 KiB (four workgroups per CU) / 16 KiB (eight)

inline int psf_lds_floats(int kh, int kw) { return (PSF_TH + kh - 1) * (PSF_TW + kw - 1); }

typedef float psf_taps4 __attribute__((ext_vector_type(4), aligned(4)));  // four taps of a row: one 4-byte aligned scalar load

// One staged row: acc[k] += t[-k * kw + b] * s[b] for K0 <= k < K1, b ascending (t: the tap row of chain 0, s: the staged row
// at this lane).  Each chain's tap row is a pointer of its own, so four taps of a row arrive in one scalar load.  The empty asm
// keeps every chain a scalar v_fmac with its tap in an SGPR: left alone, the compiler pairs two chains into a v_pk_fma_f32,
// whose tap pair (two PSF rows, one column) has to be gathered into adjacent SGPRs one s_mov at a time -- measured in the ISA
// at eight scalar instructions per packed FMA, which the one scalar issue port of a CU cannot feed.
template <int R, int K0, int K1>
__device__ __forceinline__ void psf_row(float (&acc)[R], const float* __restrict__ t, const float* s, int kw) {
  const float* tk[R];
#pragma unroll
  for (int k = K0; k < K1; ++k) tk[k] = t - k * kw;
  // Groups of four taps, two register sets in turn: the scalar loads and LDS reads of group g + 1 are issued before the
  // multiply-adds of group g, so their latency passes behind 4 (K1 - K0) FMAs and not in front of them.
  auto load = [&](psf_taps4(&tv)[R], float(&v)[4], int g) __attribute__((always_inline)) {
#pragma unroll
    for (int k = K0; k < K1; ++k) tv[k] = *reinterpret_cast<const psf_taps4*>(tk[k] + 4 * g);
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = s[4 * g + i];
  };
  auto fma4 = [&](const psf_taps4(&tv)[R], const float(&v)[4]) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
      for (int k = K0; k < K1; ++k) {
        acc[k] = __builtin_fmaf(tv[k][i], v[i], acc[k]);
        asm("" : "+v"(acc[k]));
      }
    }
  };
  const int n4 = kw / 4;
  if (n4 > 0) {
    psf_taps4 ta[R], tb[R];
    float va[4], vb[4];
    load(ta, va, 0);
    int g = 0;
    for (; g + 2 <= n4; g += 2) {
      load(tb, vb, g + 1);
      fma4(ta, va);
      load(ta, va, g + 2 < n4 ? g + 2 : n4 - 1);  // (past the end: the last group once more, not used)
      fma4(tb, vb);
    }
    if (g < n4) fma4(ta, va);  // n4 odd: group n4 - 1, loaded by the last turn (or above, n4 == 1)
  }
  for (int b = 4 * n4; b < kw; ++b) {
    const float v = s[b];
#pragma unroll
    for (int k = K0; k < K1; ++k) {
      acc[k] = __builtin_fmaf(tk[k][b], v, acc[k]);
      asm("" : "+v"(acc[k]));
    }
  }
}

template <int R, int E>
struct PsfEdge {  // the rows E .. R - 2 above the steady part (chains 0 .. E) and kh + E .. kh + R - 2 below it (chains E + 1 ..)
  static __device__ __forceinline__ void head(float (&acc)[R], const float* __restrict__ psf, const float* s, int kw, int sw) {
    if constexpr (E < R - 1) {
      psf_row<R, 0, E + 1>(acc, psf + E * kw, s + E * sw, kw);
      PsfEdge<R, E + 1>::head(acc, psf, s, kw, sw);
    }
  }
  static __device__ __forceinline__ void tail(float (&acc)[R], const float* __restrict__ psf, const float* s, int kh, int kw,
                                              int sw) {
    if constexpr (E < R - 1) {
      psf_row<R, E + 1, R>(acc, psf + (kh + E) * kw, s + (kh + E) * sw, kw);
      PsfEdge<R, E + 1>::tail(acc, psf, s, kh, kw, sw);
    }
  }
};

// The output rows i0 .. i0 + R - 1 of the tile at this lane's column; s = S + i0 * sw + lane.  kh >= R.
template <int R>
__device__ __forceinline__ void psf_block(float (&acc)[R], const float* __restrict__ psf, const float* s, int kh, int kw, int sw) {
#pragma unroll
  for (int k = 0; k < R; ++k) acc[k] = 0.f;
  PsfEdge<R, 0>::head(acc, psf, s, kw, sw);
  for (int r = R - 1; r < kh; ++r) psf_row<R, 0, R>(acc, psf + r * kw, s + r * sw, kw);
  PsfEdge<R, 0>::tail(acc, psf, s, kh, kw, sw);
}

template <int R>
__device__ __forceinline__ void psf_tile(float* __restrict__ yp, const float* __restrict__ psf, const float* S, int kh, int kw,
                                         int sw, int rows, int cols, int64_t W, int lane, int wave) {
  if (lane >= cols) return;
  for (int i0 = wave * R; i0 < rows; i0 += 4 * R) {
    float acc[R];
    psf_block<R>(acc, psf, S + i0 * sw + lane, kh, kw, sw);
#pragma unroll
    for (int k = 0; k < R; ++k)
      if (i0 + k < rows) yp[(int64_t)(i0 + k) * W + lane] = acc[k];
  }
}

template <int LDS_FLOATS, bool CIRCULAR>
__global__ __launch_bounds__(256) void op_psf_kernel(float* __restrict__ y, const float* __restrict__ x,
                                                     const float* __restrict__ psf, int kh, int kw, int64_t psf_bstride,
                                                     int64_t psf_cstride, int64_t C, int64_t H, int64_t W, int64_t tiles_y,
                                                     int64_t tiles_x, int64_t total) {
  __shared__ float S[LDS_FLOATS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int rh = kh / 2, rw = kw / 2;
  const int sw = PSF_TW + kw - 1;  // row stride of S
  for (int64_t t = blockIdx.x; t < total; t += gridDim.x) {
    const int64_t tx = t % tiles_x, q = t / tiles_x;
    const int64_t ty = q % tiles_y, plane = q / tiles_y;
    const int64_t i0 = ty * PSF_TH, j0 = tx * PSF_TW;
    const int rows = (int)(H - i0 < PSF_TH ? H - i0 : PSF_TH), cols = (int)(W - j0 < PSF_TW ? W - j0 : PSF_TW);
    const int srows = rows + kh - 1, scols = cols + kw - 1;
    const float* xp = x + plane * H * W;
    const float* k = psf + ((plane / C) * psf_bstride + (plane % C) * psf_cstride) * (kh * kw);
    // stage, as the blur does: one wrap suffices (circular: rh < H, rw < W).  A block whose last rows lie below the image reads
    // rows of S that this tile did not stage (inside the array: LDS_FLOATS holds the full tile) into chains that are not stored.
    for (int r = wave; r < srows; r += 4) {
      int64_t gy = i0 + r - rh;
      bool row_in = true;
      if (CIRCULAR) gy = gy < 0 ? gy + H : (gy >= H ? gy - H : gy);
      else row_in = gy >= 0 && gy < H;
      for (int c = lane; c < scols; c += 64) {
        int64_t gx = j0 + c - rw;
        bool in = row_in;
        if (CIRCULAR) gx = gx < 0 ? gx + W : (gx >= W ? gx - W : gx);
        else in = in && gx >= 0 && gx < W;
        S[r * sw + c] = in ? xp[gy * W + gx] : 0.f;
      }
    }
    __syncthreads();
    float* yp = y + (plane * H + i0) * W + j0;
    if (kh >= 5) psf_tile<4>(yp, k, S, kh, kw, sw, rows, cols, W, lane, wave);
    else if (kh == 3) psf_tile<2>(yp, k, S, kh, kw, sw, rows, cols, W, lane, wave);
    else psf_tile<1>(yp, k, S, kh, kw, sw, rows, cols, W, lane, wave);
    __syncthreads();  // (the next tile of this workgroup overwrites S)
  }
}

// ---------------------------------------------------------------------------------------------------------- decimation
// One thread per output pixel, adjacent lanes on adjacent j.
__global__ __launch_bounds__(256) void op_decimate_kernel(float* __restrict__ y, const float* __restrict__ x, int64_t total,
                                                          int64_t Wo, int64_t W, int fh, int fw, int oh, int ow) {
  for (int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; o < total; o += (int64_t)gridDim.x * blockDim.x) {
    const int64_t j = o % Wo, ni = o / Wo;  // ni = n * Ho + i, and input row n * H + i * fh + oh = ni * fh + oh
    y[o] = x[(ni * fh + oh) * W + j * fw + ow];
  }
}

// One thread per pixel of the large grid: every element of dx is written, the kept positions with g and the others with 0.
__global__ __launch_bounds__(256) void op_decimate_adj_kernel(float* __restrict__ dx, const float* __restrict__ g, int64_t total,
                                                              int64_t W, int64_t Wo, int fh, int fw, int oh, int ow) {
  for (int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; o < total; o += (int64_t)gridDim.x * blockDim.x) {
    const int64_t X = o % W, nY = o / W;  // nY = n * H + Y with H % fh == 0: nY % fh == Y % fh and nY / fh == n * Ho + Y / fh
    const bool kept = nY % fh == oh && X % fw == ow;
    dx[o] = kept ? g[(nY / fh) * Wo + X / fw] : 0.f;
  }
}

// --------------------------------------------------------------------------------------------------------- channel mix
// A work item is V consecutive pixels of one sample (V = 4 where HW % 4 == 0, so every plane starts 16-byte aligned; else 1).  It
// loads its Cin inputs once and forms the Cout outputs, each a chain of fused multiply-adds from 0 with c ascending.  M is
// indexed by values that are the same in every lane: it is read through the scalar cache.
constexpr int MIX_MAX = 16;

template <typename T>
__device__ __forceinline__ T mix_fma(float m, T v, T acc);
template <>
__device__ __forceinline__ float mix_fma<float>(float m, float v, float acc) { return __builtin_fmaf(m, v, acc); }
template <>
__device__ __forceinline__ float4 mix_fma<float4>(float m, float4 v, float4 acc) {
  return make_float4(__builtin_fmaf(m, v.x, acc.x), __builtin_fmaf(m, v.y, acc.y), __builtin_fmaf(m, v.z, acc.z),
                     __builtin_fmaf(m, v.w, acc.w));
}

template <typename T>  // float4 or float
__global__ __launch_bounds__(256) void op_chanmix_kernel(float* __restrict__ y, const float* __restrict__ x,
                                                         const float* __restrict__ M, int64_t total, int64_t groups, int Cin,
                                                         int Cout) {
  const T* xs = reinterpret_cast<const T*>(x);
  T* ys = reinterpret_cast<T*>(y);
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t p = i % groups, b = i / groups;  // groups: work items per plane
    T xv[MIX_MAX];
#pragma unroll
    for (int c = 0; c < MIX_MAX; ++c)
      if (c < Cin) xv[c] = xs[(b * Cin + c) * groups + p];
    for (int o = 0; o < Cout; ++o) {
      T acc = T{};
#pragma unroll
      for (int c = 0; c < MIX_MAX; ++c)
        if (c < Cin) acc = mix_fma<T>(M[o * Cin + c], xv[c], acc);
      ys[(b * Cout + o) * groups + p] = acc;
    }
  }
}

inline bool natural_f32(const void* p) { return (((uintptr_t)p) & 3u) == 0; }

inline bool overlap(const float* a, const float* b, int64_t n) { return a < b + n && b < a + n; }

inline bool overlap2(const float* a, int64_t na, const float* b, int64_t nb) { return a < b + nb && b < a + na; }

inline bool psf_size_ok(int32_t kh, int32_t kw) { return kh >= 1 && kh <= PSF_MAX && (kh & 1) && kw >= 1 && kw <= PSF_MAX && (kw & 1); }

inline bool decimate_ok(int64_t planes, int64_t H, int64_t W, int32_t fh, int32_t fw, int32_t oh, int32_t ow) {
  return planes > 0 && H > 0 && W > 0 && fh >= 1 && fh <= 16 && fw >= 1 && fw <= 16 && oh >= 0 && oh < fh && ow >= 0 && ow < fw &&
         H % fh == 0 && W % fw == 0 && planes <= INT64_MAX / H / W;
}

}  // namespace

extern "C" {

int az_op_mul_f32(float* y, const float* x, const float* m, int64_t n, int64_t m_n, az_stream_t stream) {
  AZ_REQUIRE(y && x && m, AZ_E_NULL);
  AZ_REQUIRE(n > 0 && m_n > 0 && m_n <= n && n % m_n == 0, AZ_E_SHAPE);
  AZ_REQUIRE(AZ_ALIGNED16(y) && AZ_ALIGNED16(x) && AZ_ALIGNED16(m), AZ_E_ALIGN);
  const int grid = az_stream_grid(n / 4, 256);
  if (m_n % 4 == 0) hipLaunchKernelGGL(op_mul_kernel<true>, dim3(grid), dim3(256), 0, az_s(stream), y, x, m, n, m_n);
  else hipLaunchKernelGGL(op_mul_kernel<false>, dim3(grid), dim3(256), 0, az_s(stream), y, x, m, n, m_n);
  return az_launch_status();
}

int az_op_avgpool_f32(float* y, const float* x, int64_t planes, int64_t H, int64_t W, int32_t fh, int32_t fw,
                      az_stream_t stream) {
  AZ_REQUIRE(y && x, AZ_E_NULL);
  AZ_REQUIRE(planes > 0 && H > 0 && W > 0 && fh >= 1 && fh <= 16 && fw >= 1 && fw <= 16, AZ_E_SHAPE);
  AZ_REQUIRE(H % fh == 0 && W % fw == 0, AZ_E_SHAPE);
  AZ_REQUIRE(AZ_ALIGNED16(y) && AZ_ALIGNED16(x), AZ_E_ALIGN);
  const int64_t Ho = H / fh, Wo = W / fw, total = planes * Ho * Wo;
  const float inv = (float)(1.0 / (double)(fh * fw));
  hipLaunchKernelGGL(op_avgpool_kernel, dim3(az_stream_grid(total, 256)), dim3(256), 0, az_s(stream), y, x, total, Ho, Wo, W,
                     (int)fh, (int)fw, inv);
  return az_launch_status();
}

int az_op_avgpool_adj_f32(float* dx, const float* g, int64_t planes, int64_t H, int64_t W, int32_t fh, int32_t fw, float scale,
                          az_stream_t stream) {
  AZ_REQUIRE(dx && g, AZ_E_NULL);
  AZ_REQUIRE(planes > 0 && H > 0 && W > 0 && fh >= 1 && fh <= 16 && fw >= 1 && fw <= 16, AZ_E_SHAPE);
  AZ_REQUIRE(H % fh == 0 && W % fw == 0, AZ_E_SHAPE);
  AZ_REQUIRE(AZ_ALIGNED16(dx) && AZ_ALIGNED16(g), AZ_E_ALIGN);
  const int64_t total = planes * H * W;
  hipLaunchKernelGGL(op_avgpool_adj_kernel, dim3(az_stream_grid(total, 256)), dim3(256), 0, az_s(stream), dx, g, total, H, W,
                     W / fw, (int)fh, (int)fw, scale);
  return az_launch_status();
}

int az_op_blur_tile(int32_t nh, int32_t nw, int32_t* th, int32_t* tw) {
  AZ_REQUIRE(th && tw, AZ_E_NULL);
  AZ_REQUIRE(nh >= 1 && nh <= BLUR_MAX_TAPS && (nh & 1) && nw >= 1 && nw <= BLUR_MAX_TAPS && (nw & 1), AZ_E_SHAPE);
  *th = blur_tile_rows(nh, nw);
  *tw = BLUR_TW;
  return AZ_OK;
}

int az_op_blur_f32(float* y, const float* x, const float* taps_h, int32_t nh, const float* taps_w, int32_t nw, int64_t planes,
                   int64_t H, int64_t W, int32_t circular, az_stream_t stream) {
  AZ_REQUIRE(y && x && taps_h && taps_w, AZ_E_NULL);
  AZ_REQUIRE(nh >= 1 && nh <= BLUR_MAX_TAPS && (nh & 1) && nw >= 1 && nw <= BLUR_MAX_TAPS && (nw & 1), AZ_E_SHAPE);
  AZ_REQUIRE(planes > 0 && H > 0 && W > 0 && (circular == 0 || circular == 1), AZ_E_SHAPE);
  AZ_REQUIRE(planes <= INT64_MAX / H / W, AZ_E_SHAPE);
  AZ_REQUIRE(!circular || (nh / 2 < H && nw / 2 < W), AZ_E_SHAPE);
  AZ_REQUIRE(!overlap(y, x, planes * H * W), AZ_E_SHAPE);  // a tile reads the halo its neighbours write: never in place
  AZ_REQUIRE(AZ_ALIGNED16(y) && AZ_ALIGNED16(x) && natural_f32(taps_h) && natural_f32(taps_w), AZ_E_ALIGN);
  const int th = blur_tile_rows(nh, nw);
  const int64_t tiles_y = (H + th - 1) / th, tiles_x = (W + BLUR_TW - 1) / BLUR_TW, total = planes * tiles_y * tiles_x;
  const int grid = (int)(total < (1 << 20) ? total : (1 << 20));
  const bool small = blur_lds_floats(th, nh, nw) <= BLUR_LDS_SMALL;
#define AZ_BLUR(L, CIRC)                                                                                                    \
  hipLaunchKernelGGL((op_blur_kernel<L, CIRC>), dim3(grid), dim3(256), 0, az_s(stream), y, x, taps_h, (int)nh, taps_w, (int)nw, H, \
                     W, th, tiles_y, tiles_x, total)
  if (small && circular) AZ_BLUR(BLUR_LDS_SMALL, true);
  else if (small) AZ_BLUR(BLUR_LDS_SMALL, false);
  else if (circular) AZ_BLUR(BLUR_LDS_BIG, true);
  else AZ_BLUR(BLUR_LDS_BIG, false);
#undef AZ_BLUR
  return az_launch_status();
}

int az_op_psf_tile(int32_t kh, int32_t kw, int32_t* th, int32_t* tw) {
  AZ_REQUIRE(th && tw, AZ_E_NULL);
  AZ_REQUIRE(psf_size_ok(kh, kw), AZ_E_SHAPE);
  *th = PSF_TH;
  *tw = PSF_TW;
  return AZ_OK;
}

int az_op_psf_f32(float* y, const float* x, const float* psf, int32_t kh, int32_t kw, int64_t psf_bstride, int64_t psf_cstride,
                  int64_t B, int64_t C, int64_t H, int64_t W, int32_t circular, az_stream_t stream) {
  AZ_REQUIRE(y && x && psf, AZ_E_NULL);
  AZ_REQUIRE(psf_size_ok(kh, kw) && psf_bstride >= 0 && psf_cstride >= 0, AZ_E_SHAPE);
  AZ_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0 && (circular == 0 || circular == 1), AZ_E_SHAPE);
  AZ_REQUIRE(B <= INT64_MAX / C && B * C <= INT64_MAX / H / W, AZ_E_SHAPE);
  AZ_REQUIRE(psf_bstride <= (INT64_MAX >> 13) / B && psf_cstride <= (INT64_MAX >> 13) / C, AZ_E_SHAPE);  // (kh kw < 2^13)
  AZ_REQUIRE(!circular || (kh / 2 < H && kw / 2 < W), AZ_E_SHAPE);
  AZ_REQUIRE(!overlap(y, x, B * C * H * W), AZ_E_SHAPE);  // a tile reads the halo its neighbours write: never in place
  AZ_REQUIRE(AZ_ALIGNED16(y) && AZ_ALIGNED16(x) && natural_f32(psf), AZ_E_ALIGN);
  const int64_t tiles_y = (H + PSF_TH - 1) / PSF_TH, tiles_x = (W + PSF_TW - 1) / PSF_TW, total = B * C * tiles_y * tiles_x;
  const int grid = (int)(total < (1 << 16) ? total : (1 << 16));
  const bool small = psf_lds_floats(kh, kw) <= PSF_LDS_SMALL;
#define AZ_PSF(L, CIRC)                                                                                                      \
  hipLaunchKernelGGL((op_psf_kernel<L, CIRC>), dim3(grid), dim3(256), 0, az_s(stream), y, x, psf, (int)kh, (int)kw, psf_bstride, \
                     psf_cstride, C, H, W, tiles_y, tiles_x, total)
  if (small && circular) AZ_PSF(PSF_LDS_SMALL, true);
  else if (small) AZ_PSF(PSF_LDS_SMALL, false);
  else if (circular) AZ_PSF(PSF_LDS_BIG, true);
  else AZ_PSF(PSF_LDS_BIG, false);
#undef AZ_PSF
  return az_launch_status();
}

int az_op_decimate_f32(float* y, const float* x, int64_t planes, int64_t H, int64_t W, int32_t fh, int32_t fw, int32_t oh,
                       int32_t ow, az_stream_t stream) {
  AZ_REQUIRE(y && x, AZ_E_NULL);
  AZ_REQUIRE(decimate_ok(planes, H, W, fh, fw, oh, ow), AZ_E_SHAPE);
  const int64_t Ho = H / fh, Wo = W / fw, total = planes * Ho * Wo;
  AZ_REQUIRE(!overlap2(y, total, x, planes * H * W), AZ_E_SHAPE);
  AZ_REQUIRE(AZ_ALIGNED16(y) && AZ_ALIGNED16(x), AZ_E_ALIGN);
  hipLaunchKernelGGL(op_decimate_kernel, dim3(az_stream_grid(total, 256)), dim3(256), 0, az_s(stream), y, x, total, Wo, W, (int)fh,
                     (int)fw, (int)oh, (int)ow);
  return az_launch_status();
}

int az_op_decimate_adj_f32(float* dx, const float* g, int64_t planes, int64_t H, int64_t W, int32_t fh, int32_t fw, int32_t oh,
                           int32_t ow, az_stream_t stream) {
  AZ_REQUIRE(dx && g, AZ_E_NULL);
  AZ_REQUIRE(decimate_ok(planes, H, W, fh, fw, oh, ow), AZ_E_SHAPE);
  const int64_t total = planes * H * W;
  AZ_REQUIRE(!overlap2(dx, total, g, planes * (H / fh) * (W / fw)), AZ_E_SHAPE);
  AZ_REQUIRE(AZ_ALIGNED16(dx) && AZ_ALIGNED16(g), AZ_E_ALIGN);
  hipLaunchKernelGGL(op_decimate_adj_kernel, dim3(az_stream_grid(total, 256)), dim3(256), 0, az_s(stream), dx, g, total, W, W / fw,
                     (int)fh, (int)fw, (int)oh, (int)ow);
  return az_launch_status();
}

int az_op_chanmix_f32(float* y, const float* x, const float* M, int64_t B, int32_t Cin, int32_t Cout, int64_t HW,
                      az_stream_t stream) {
  AZ_REQUIRE(y && x && M, AZ_E_NULL);
  AZ_REQUIRE(B > 0 && HW > 0 && Cin >= 1 && Cin <= MIX_MAX && Cout >= 1 && Cout <= MIX_MAX, AZ_E_SHAPE);
  AZ_REQUIRE(B <= INT64_MAX / MIX_MAX / HW, AZ_E_SHAPE);
  AZ_REQUIRE(!overlap2(y, B * Cout * HW, x, B * Cin * HW), AZ_E_SHAPE);  // an output plane is written before others read x
  AZ_REQUIRE(AZ_ALIGNED16(y) && AZ_ALIGNED16(x) && natural_f32(M), AZ_E_ALIGN);
  if (HW % 4 == 0) {
    const int64_t groups = HW / 4, total = B * groups;
    hipLaunchKernelGGL(op_chanmix_kernel<float4>, dim3(az_stream_grid(total, 256)), dim3(256), 0, az_s(stream), y, x, M, total,
                       groups, (int)Cin, (int)Cout);
  } else {
    const int64_t total = B * HW;
    hipLaunchKernelGGL(op_chanmix_kernel<float>, dim3(az_stream_grid(total, 256)), dim3(256), 0, az_s(stream), y, x, M, total, HW,
                       (int)Cin, (int)Cout);
  }
  return az_launch_status();
}

}  // extern "C"
