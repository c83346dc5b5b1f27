// Batched 2-D complex DFT of the Fourier-domain measurement operators (azula_amd/guidance/operators.py: FourierOperator,
// MRIOperator).  Planes of H x W fp32 in SPLIT-complex form: the real and the imaginary parts are separate planes, plane (b, c)
// of a tensor at base + b * bstride + c * H * W.  H and W are powers of two, 1 .. 1024.
//
//   az_op_fft2_f32   dst[k, l] = scale * sum_{m, n} src[m, n] exp(-+ 2 pi i (k m / H + l n / W))
//
// A workgroup holds up to P complex points in LDS (P = 8192: 64 KiB, 1024 threads; P = 1024: 8 KiB, 256 threads) and runs
// Stockham stages on them: radix 4, after one radix-2 stage where log2 n is odd.  A stage is   read R points per item ->
// twiddle -> butterfly in registers -> barrier -> write the R results -> barrier,   in place: every read of a stage precedes
// every write, so one buffer serves.  Three forms, chosen on the host from H W alone:
//
//   whole   H W <= P: the plane is loaded once, transformed along its rows and then along its columns in LDS, and stored.
//           4 or 8 B read and 4 or 8 B written per element, one launch.
//   rows    H W > 8192, first launch: a tile is P / W consecutive rows (P consecutive floats of the plane); src -> mid.
//   cols    second launch: a tile is T = P / H adjacent columns x H rows, every global access a run of T floats of a row;
//           mid -> dst in place (a tile reads all it owns before it writes).  mid is dst_re and dst_im (or `work` when dst_im is
//           NULL).  4 + 8 B, then 8 + 8 B per element for real -> complex: 28 B.
//
// LDS index g of point i of line l: rows g = l n + i, columns g = i T + c -- the plane (or tile) in row-major order both times.
// Lanes run along the contiguous axis.  Stockham reads (points j + r n / R) are then consecutive words, but the writes of the
// early stages (points (j / Ns) Ns R + j % Ns + r Ns) walk strides of R, so g is swizzled: fft_sw XORs bits 0 .. 4 with
// 0b10101 where bit 5 is set and with 0b11010 where bit 6 is set.  Over GF(2) this map is injective on each set of five address
// bits that the 32 lanes of a half wave vary in a row stage ({2..6}, {0,1,4,5,6}, {0..3,6} for even log2 n; {1..5}, {0,3..6},
// {0,1,2,5,6} for odd; {0..4} for every read, load and store), so ds_read_b32 / ds_write_b32 (banks modulo 32, groups of 32
// lanes) are conflict free there; DESIGN.md section 9d has the table and the column cases.
//
// Twiddles are sincospif of the exact fraction r k / (Ns R / 2) (a product of small integers and a power of two: exact in
// fp32): about one ulp, and exactly 0 / +-1 at multiples of a quarter turn, so H, W <= 4 are exact on integer data.
// No atomics, a fixed order of operations, nothing that depends on the plane count or the plane's place in the launch; int64
// offsets; tiles are a linear range walked with a grid stride; the caller's stream.
#include "common.h"

namespace {

constexpr int FFT_MAX = AZ_OP_FFT2_MAX;
constexpr int FFT_LP_BIG = 13;
constexpr int FFT_P_BIG = 1 << FFT_LP_BIG, FFT_P_SMALL = 1024;  // complex points of LDS per workgroup
constexpr int FFT_TH_BIG = 1024, FFT_TH_SMALL = 256;  // threads of a workgroup that holds FFT_P_BIG / FFT_P_SMALL points

__device__ __forceinline__ int fft_sw(int g) { return g ^ (((g >> 5) & 1) * 21) ^ (((g >> 6) & 1) * 26); }

// One Stockham stage of radix R over all lines in LDS.  n = 1 << ln points per line, Ns = 1 << lns the product of the radices of
// the stages before, 1 << ltot points in all.  cols: point i of line c sits at i << lt + c (lines are the 1 << lt columns);
// otherwise at l << ln + i.  dir: -1 forward, +1 inverse.
template <int P, int TH, int R>
__device__ __forceinline__ void fft_stage(float* re, float* im, int tid, int ln, int lns, int lt, bool cols, int ltot, float dir) {
  constexpr int LR = R == 4 ? 2 : 1;
  constexpr int ITEMS = (P / R + TH - 1) / TH;
  const int items = 1 << (ltot - LR), lq = ln - LR, es = cols ? lt : 0;
  const float inv = dir / (float)(1 << (lns + LR - 1));  // (r k) * inv: the angle in half turns, exact
  float vr[ITEMS][R], vi[ITEMS][R];
#pragma unroll
  for (int it = 0; it < ITEMS; ++it) {
    const int q = it * TH + tid;
    if (q < items) {
      const int j = cols ? q >> lt : q & ((1 << lq) - 1);
      const int base = cols ? q & ((1 << lt) - 1) : (q >> lq) << ln;
      const int k = j & ((1 << lns) - 1);
      float xr[R], xi[R];
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const int g = fft_sw(base + ((j + (r << lq)) << es));
        xr[r] = re[g];
        xi[r] = im[g];
      }
#pragma unroll
      for (int r = 1; r < R; ++r) {
        float s, c;
        sincospif((float)(r * k) * inv, &s, &c);
        const float a = xr[r], b = xi[r];
        xr[r] = __builtin_fmaf(a, c, -az_mul(b, s));
        xi[r] = __builtin_fmaf(a, s, az_mul(b, c));
      }
      if (R == 2) {
        vr[it][0] = az_add(xr[0], xr[1]);
        vi[it][0] = az_add(xi[0], xi[1]);
        vr[it][1] = az_sub(xr[0], xr[1]);
        vi[it][1] = az_sub(xi[0], xi[1]);
      } else {
        const float a0r = az_add(xr[0], xr[2]), a0i = az_add(xi[0], xi[2]);
        const float a1r = az_sub(xr[0], xr[2]), a1i = az_sub(xi[0], xi[2]);
        const float a2r = az_add(xr[1], xr[3]), a2i = az_add(xi[1], xi[3]);
        const float dr = az_sub(xr[1], xr[3]), di = az_sub(xi[1], xi[3]);
        const float a3r = dir < 0.f ? di : -di, a3i = dir < 0.f ? -dr : dr;  // (x1 - x3) * (dir i)
        vr[it][0] = az_add(a0r, a2r);
        vi[it][0] = az_add(a0i, a2i);
        vr[it][1] = az_add(a1r, a3r);
        vi[it][1] = az_add(a1i, a3i);
        vr[it][2] = az_sub(a0r, a2r);
        vi[it][2] = az_sub(a0i, a2i);
        vr[it][R - 1] = az_sub(a1r, a3r);
        vi[it][R - 1] = az_sub(a1i, a3i);
      }
    }
  }
  __syncthreads();
#pragma unroll
  for (int it = 0; it < ITEMS; ++it) {
    const int q = it * TH + tid;
    if (q < items) {
      const int j = cols ? q >> lt : q & ((1 << lq) - 1);
      const int base = cols ? q & ((1 << lt) - 1) : (q >> lq) << ln;
      const int i0 = ((j >> lns) << (lns + LR)) + (j & ((1 << lns) - 1));
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const int g = fft_sw(base + ((i0 + (r << lns)) << es));
        re[g] = vr[it][r];
        im[g] = vi[it][r];
      }
    }
  }
  __syncthreads();
}

// The 1 << (ltot - ln) lines of 1 << ln points in LDS, each transformed in place.  Called by all threads, after a barrier.
template <int P, int TH>
__device__ __forceinline__ void fft_lines(float* re, float* im, int tid, int ln, int lt, bool cols, int ltot, float dir) {
  int lns = 0;
  if (ln & 1) {
    fft_stage<P, TH, 2>(re, im, tid, ln, 0, lt, cols, ltot, dir);
    lns = 1;
  }
  for (; lns < ln; lns += 2) fft_stage<P, TH, 4>(re, im, tid, ln, lns, lt, cols, ltot, dir);
}

struct FftArgs {
  float* dst_re;
  float* dst_im;  // NULL: not written
  int64_t dst_bs, dst_im_bs;
  const float* src_re;
  const float* src_im;  // NULL: zero
  int64_t src_bs, src_im_bs;
  int64_t C, total;  // total: tiles of the launch
  int lh, lw;
  float dir, scale;
};

enum { FFT_WHOLE = 0, FFT_ROWS = 1, FFT_COLS = 2 };

// FFT_WHOLE: a tile is a plane.  FFT_ROWS: P consecutive floats of a plane (P / W rows), no scale.  FFT_COLS: P / H columns.
template <int P, int TH, int MODE>
__global__ __launch_bounds__(TH) void fft2_kernel(FftArgs a) {
  __shared__ float re[P], im[P];
  const int tid = threadIdx.x;
  const int lhw = a.lh + a.lw;
  const int64_t HW = (int64_t)1 << lhw, W = (int64_t)1 << a.lw;
  // tiles per plane, points per tile, and (FFT_COLS) log2 of the tile's width
  const int ltpp = MODE == FFT_WHOLE ? 0 : lhw - FFT_LP_BIG, lt = MODE == FFT_COLS ? FFT_LP_BIG - a.lh : 0;
  const int ltot = MODE == FFT_WHOLE ? lhw : FFT_LP_BIG;
  const int npts = 1 << ltot;
  for (int64_t t = blockIdx.x; t < a.total; t += gridDim.x) {
    const int64_t plane = t >> ltpp, chunk = t & (((int64_t)1 << ltpp) - 1);
    const int64_t b = plane / a.C, c = plane % a.C;
    const int64_t so = b * a.src_bs + c * HW, dof = b * a.dst_bs + c * HW;
    const int64_t sio = b * a.src_im_bs + c * HW, dio = b * a.dst_im_bs + c * HW;  // (the imaginary planes)
    if (MODE == FFT_COLS) {  // global element of LDS word g = r T + cc: row r, column chunk T + cc
      const int64_t c0 = chunk << lt;
      for (int g = tid; g < npts; g += TH) {
        const int64_t e = (int64_t)(g >> lt) * W + c0 + (g & ((1 << lt) - 1));
        re[fft_sw(g)] = a.src_re[so + e];
        im[fft_sw(g)] = a.src_im[sio + e];
      }
    } else {
      const int64_t e0 = chunk << FFT_LP_BIG;
      for (int g = tid; g < npts; g += TH) {
        re[fft_sw(g)] = a.src_re[so + e0 + g];
        im[fft_sw(g)] = a.src_im ? a.src_im[sio + e0 + g] : 0.f;
      }
    }
    __syncthreads();
    if (MODE != FFT_COLS) fft_lines<P, TH>(re, im, tid, a.lw, 0, false, ltot, a.dir);
    if (MODE == FFT_WHOLE) fft_lines<P, TH>(re, im, tid, a.lh, a.lw, true, ltot, a.dir);
    if (MODE == FFT_COLS) fft_lines<P, TH>(re, im, tid, a.lh, lt, true, ltot, a.dir);
    if (MODE == FFT_COLS) {
      const int64_t c0 = chunk << lt;
      for (int g = tid; g < npts; g += TH) {
        const int64_t e = (int64_t)(g >> lt) * W + c0 + (g & ((1 << lt) - 1));
        a.dst_re[dof + e] = az_mul(a.scale, re[fft_sw(g)]);
        if (a.dst_im) a.dst_im[dio + e] = az_mul(a.scale, im[fft_sw(g)]);
      }
    } else {
      const int64_t e0 = chunk << FFT_LP_BIG;
      for (int g = tid; g < npts; g += TH) {
        a.dst_re[dof + e0 + g] = MODE == FFT_ROWS ? re[fft_sw(g)] : az_mul(a.scale, re[fft_sw(g)]);
        if (a.dst_im) a.dst_im[dio + e0 + g] = MODE == FFT_ROWS ? im[fft_sw(g)] : az_mul(a.scale, im[fft_sw(g)]);
      }
    }
    __syncthreads();  // (the next tile of this workgroup overwrites re and im)
  }
}

inline int fft_log2(int32_t n) {  // log2 of a power of two in 1 .. FFT_MAX, else -1
  if (n < 1 || n > FFT_MAX || (n & (n - 1))) return -1;
  int l = 0;
  while ((1 << l) < n) ++l;
  return l;
}

inline bool fft_shape_ok(int64_t B, int64_t C, int32_t H, int32_t W) {
  return B > 0 && C > 0 && fft_log2(H) >= 0 && fft_log2(W) >= 0 && B <= (INT64_MAX >> 22) / C;  // (B C H W and twice that fit)
}

// The planes p + b * bs + [0, n) floats, b < B, of two tensors share no float.  Tensors of one stride may interleave (the two
// halves of a (B, 2 C, H, W) tensor); anything else has to lie apart as a whole.
inline bool fft_disjoint(const float* p, int64_t ps, const float* q, int64_t qs, int64_t B, int64_t n, int64_t qn) {
  const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
  const uint64_t ea = (uint64_t)((B - 1) * ps + n) * 4, eb = (uint64_t)((B - 1) * qs + qn) * 4;
  if (a + ea <= b || b + eb <= a) return true;
  if (B == 1 || ps != qs || n != qn) return false;
  const uint64_t r = (a > b ? a - b : b - a) % ((uint64_t)ps * 4);
  return r >= (uint64_t)n * 4 && r + (uint64_t)n * 4 <= (uint64_t)ps * 4;
}

}  // namespace

extern "C" {

int az_op_fft2_work(int64_t B, int64_t C, int32_t H, int32_t W, int64_t* floats) {
  AZ_REQUIRE(floats, AZ_E_NULL);
  AZ_REQUIRE(fft_shape_ok(B, C, H, W), AZ_E_SHAPE);
  *floats = (int64_t)H * W <= FFT_P_BIG ? 0 : B * C * H * W;
  return AZ_OK;
}

int az_op_fft2_f32(float* dst_re, float* dst_im, int64_t dst_bstride, const float* src_re, const float* src_im,
                   int64_t src_bstride, float* work, int64_t B, int64_t C, int32_t H, int32_t W, int32_t inverse, float scale,
                   az_stream_t stream) {
  AZ_REQUIRE(dst_re && src_re, AZ_E_NULL);
  AZ_REQUIRE(fft_shape_ok(B, C, H, W) && (inverse == 0 || inverse == 1), AZ_E_SHAPE);
  const int64_t HW = (int64_t)H * W, n = C * HW;
  const bool whole = HW <= FFT_P_BIG, need_work = !whole && !dst_im;
  AZ_REQUIRE(!need_work || work, AZ_E_NULL);
  AZ_REQUIRE(dst_bstride >= (B > 1 ? n : 0) && src_bstride >= (B > 1 ? n : 0), AZ_E_SHAPE);  // a tensor's own planes lie apart
  AZ_REQUIRE(dst_bstride <= (INT64_MAX >> 3) / B && src_bstride <= (INT64_MAX >> 3) / B, AZ_E_SHAPE);
  AZ_REQUIRE(AZ_ALIGNED16(dst_re) && AZ_ALIGNED16(dst_im) && AZ_ALIGNED16(src_re) && AZ_ALIGNED16(src_im) &&
                 (!need_work || AZ_ALIGNED16(work)),
             AZ_E_ALIGN);
  // nothing is transformed in place: a workgroup writes where others still read
  AZ_REQUIRE(fft_disjoint(dst_re, dst_bstride, src_re, src_bstride, B, n, n), AZ_E_SHAPE);
  AZ_REQUIRE(!src_im || fft_disjoint(dst_re, dst_bstride, src_im, src_bstride, B, n, n), AZ_E_SHAPE);
  AZ_REQUIRE(!src_im || fft_disjoint(src_re, src_bstride, src_im, src_bstride, B, n, n), AZ_E_SHAPE);
  if (dst_im) {
    AZ_REQUIRE(fft_disjoint(dst_im, dst_bstride, dst_re, dst_bstride, B, n, n), AZ_E_SHAPE);
    AZ_REQUIRE(fft_disjoint(dst_im, dst_bstride, src_re, src_bstride, B, n, n), AZ_E_SHAPE);
    AZ_REQUIRE(!src_im || fft_disjoint(dst_im, dst_bstride, src_im, src_bstride, B, n, n), AZ_E_SHAPE);
  }
  if (need_work) {  // B * n dense floats
    AZ_REQUIRE(fft_disjoint(dst_re, dst_bstride, work, 0, B, n, B * n), AZ_E_SHAPE);
    AZ_REQUIRE(fft_disjoint(src_re, src_bstride, work, 0, B, n, B * n), AZ_E_SHAPE);
    AZ_REQUIRE(!src_im || fft_disjoint(src_im, src_bstride, work, 0, B, n, B * n), AZ_E_SHAPE);
  }
  FftArgs a;
  a.dst_re = dst_re, a.dst_im = dst_im, a.dst_bs = a.dst_im_bs = dst_bstride;
  a.src_re = src_re, a.src_im = src_im, a.src_bs = a.src_im_bs = src_bstride;
  a.C = C, a.lh = fft_log2(H), a.lw = fft_log2(W);
  a.dir = inverse ? 1.f : -1.f, a.scale = scale;
  const int64_t planes = B * C;
  auto grid = [](int64_t total) { return dim3((unsigned)(total < 4096 ? total : 4096)); };
  if (whole) {
    a.total = planes;
    if (HW <= FFT_P_SMALL)
      hipLaunchKernelGGL((fft2_kernel<FFT_P_SMALL, FFT_TH_SMALL, FFT_WHOLE>), grid(a.total), dim3(FFT_TH_SMALL), 0, az_s(stream), a);
    else hipLaunchKernelGGL((fft2_kernel<FFT_P_BIG, FFT_TH_BIG, FFT_WHOLE>), grid(a.total), dim3(FFT_TH_BIG), 0, az_s(stream), a);
    return az_launch_status();
  }
  // rows: src -> mid, where mid is dst_re with dst_im, or with the dense `work` where the caller wants no imaginary part
  a.total = planes * (HW / FFT_P_BIG);
  FftArgs r = a;
  if (!dst_im) r.dst_im = work, r.dst_im_bs = n;
  hipLaunchKernelGGL((fft2_kernel<FFT_P_BIG, FFT_TH_BIG, FFT_ROWS>), grid(r.total), dim3(FFT_TH_BIG), 0, az_s(stream), r);
  int rc = az_launch_status();
  if (rc != AZ_OK) return rc;
  FftArgs c = a;  // cols: mid -> dst, in place on dst_re (and dst_im)
  c.src_re = dst_re, c.src_im = r.dst_im, c.src_bs = dst_bstride, c.src_im_bs = r.dst_im_bs;
  hipLaunchKernelGGL((fft2_kernel<FFT_P_BIG, FFT_TH_BIG, FFT_COLS>), grid(c.total), dim3(FFT_TH_BIG), 0, az_s(stream), c);
  return az_launch_status();
}

}  // extern "C"
