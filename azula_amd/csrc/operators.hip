// Measurement operators of the guidance methods (azula_amd/guidance/operators.py): pixel mask, average-pool downsampling with
// its adjoint / pseudo-inverse, and a separable blur.  Planar fp32 (B, C, H, W) tensors seen as planes = B * C images of H x W.
//
//   az_op_mul_f32          y[i] = x[i] * m[i mod m_n]                                   8 B / element (+ m, cache resident)
//   az_op_avgpool_f32      y[n, i, j] = (sum_{a, b} x[n, i fh + a, j fw + b]) / (fh fw)  4 + 4 / (fh fw) B / input element
//   az_op_avgpool_adj_f32  dx[n, Y, X] = scale * g[n, Y / fh, X / fw]                    4 + 4 / (fh fw) B / output element
//   az_op_blur_f32         y = taps_h (x) taps_w correlated with x, zero or wrapped edge 8 B / element from HBM (halo: L2)
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

inline bool natural_f32(const void* p) { return (((uintptr_t)p) & 3u) == 0; }

inline bool overlap(const float* a, const float* b, int64_t n) { return a < b + n && b < a + n; }

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

}  // extern "C"
