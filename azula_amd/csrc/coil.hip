// The coil maps of multi-coil (SENSE) MRI (azula_amd/guidance/operators.py: MultiCoilMRIOperator): y_k = M F (S_k . x) with
// complex sensitivity maps S_k.  SPLIT-complex fp32 in az_op_fft2_f32's plane convention: plane (b, k) of a tensor starts at
// base + b * bstride + k * HW floats, the real and the imaginary parts have separate bases.
//
//   az_op_coil_expand_f32   dst[b, k] = S[b, k] . x[b]                    (4 or 8) + 16 K bytes / pixel
//   az_op_coil_combine_f32  dst[b] = sum_k conj(S[b, k]) . z[b, k]        16 K + (4 or 8) bytes / pixel
//                           (normalize: divided by sum_k |S[b, k]|^2, 0 where that is 0; the maps are read anyway)
//
// One work item owns 4 consecutive pixels of one sample and walks the K coils: x (expand) or the accumulators (combine) stay in
// registers, so x is read once and the combined image written once, whatever K.  Items are a linear int64 range walked with a
// grid stride by a capped grid.  No atomics, coils in ascending order: two launches on the same data give the same bits, and a
// sample's result does not depend on the other samples of the launch.
//
// Arithmetic.  expand, x = a + i b, S = c + i d: re = fma(a, c, -(b d)), im = fma(a, d, b c) (the product form of fft.hip's
// twiddles); a real image gives re = a c, im = a d, single roundings.  combine, z = p + i q, from 0 with k ascending:
// re = fma(c, p, re), re = fma(d, q, re); im = fma(c, q, im), im = fma(-d, p, im); D = fma(c, c, D), D = fma(d, d, D).
#include "common.h"

namespace {

constexpr int COIL_BLOCK = 256, COIL_GRID = 1024;  // 256 CUs x 4 workgroups: 16 waves per CU, each with 4+ 16-byte loads in flight

struct CoilArgs {
  float* dst_re;
  float* dst_im;  // combine: NULL = real part only
  int64_t dst_bs;
  const float* src_re;  // expand: x; combine: z
  const float* src_im;  // expand: NULL = real image
  int64_t src_bs;
  const float* s_re;
  const float* s_im;
  int64_t s_bs;
  int64_t HW, groups, total;  // groups = ceil(HW / 4) items per sample, total = B * groups
  int K;
};

// V4: every base and stride is a multiple of 4 floats and HW % 4 == 0, so an item is one aligned float4 per plane.  Otherwise the
// item's (up to) 4 pixels go one by one; `n` of them lie inside the plane.
template <bool V4>
__device__ __forceinline__ float4 coil_ld(const float* p, int n) {
  if (V4) return *reinterpret_cast<const float4*>(p);
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  v.x = p[0];
  if (n > 1) v.y = p[1];
  if (n > 2) v.z = p[2];
  if (n > 3) v.w = p[3];
  return v;
}
template <bool V4>
__device__ __forceinline__ void coil_st(float* p, float4 v, int n) {
  if (V4) {
    *reinterpret_cast<float4*>(p) = v;
    return;
  }
  p[0] = v.x;
  if (n > 1) p[1] = v.y;
  if (n > 2) p[2] = v.z;
  if (n > 3) p[3] = v.w;
}

#define COIL_EACH(expr_x, expr_y, expr_z, expr_w) make_float4(expr_x, expr_y, expr_z, expr_w)

template <bool V4, bool XIM>
__global__ __launch_bounds__(COIL_BLOCK) void coil_expand_kernel(CoilArgs g) {
  for (int64_t i = (int64_t)blockIdx.x * COIL_BLOCK + threadIdx.x; i < g.total; i += (int64_t)gridDim.x * COIL_BLOCK) {
    const int64_t b = i / g.groups, e = (i - b * g.groups) * 4;
    const int n = g.HW - e < 4 ? (int)(g.HW - e) : 4;
    const float4 a = coil_ld<V4>(g.src_re + b * g.src_bs + e, n);
    float4 bi = make_float4(0.f, 0.f, 0.f, 0.f);
    if (XIM) bi = coil_ld<V4>(g.src_im + b * g.src_bs + e, n);
    const float* sr = g.s_re + b * g.s_bs + e;
    const float* si = g.s_im + b * g.s_bs + e;
    float* dr = g.dst_re + b * g.dst_bs + e;
    float* di = g.dst_im + b * g.dst_bs + e;
#pragma unroll 2
    for (int k = 0; k < g.K; ++k) {
      const int64_t o = (int64_t)k * g.HW;
      const float4 c = coil_ld<V4>(sr + o, n), d = coil_ld<V4>(si + o, n);
      float4 re, im;
      if (XIM) {
        re = COIL_EACH(__builtin_fmaf(a.x, c.x, -az_mul(bi.x, d.x)), __builtin_fmaf(a.y, c.y, -az_mul(bi.y, d.y)),
                       __builtin_fmaf(a.z, c.z, -az_mul(bi.z, d.z)), __builtin_fmaf(a.w, c.w, -az_mul(bi.w, d.w)));
        im = COIL_EACH(__builtin_fmaf(a.x, d.x, az_mul(bi.x, c.x)), __builtin_fmaf(a.y, d.y, az_mul(bi.y, c.y)),
                       __builtin_fmaf(a.z, d.z, az_mul(bi.z, c.z)), __builtin_fmaf(a.w, d.w, az_mul(bi.w, c.w)));
      } else {
        re = COIL_EACH(az_mul(a.x, c.x), az_mul(a.y, c.y), az_mul(a.z, c.z), az_mul(a.w, c.w));
        im = COIL_EACH(az_mul(a.x, d.x), az_mul(a.y, d.y), az_mul(a.z, d.z), az_mul(a.w, d.w));
      }
      coil_st<V4>(dr + o, re, n);
      coil_st<V4>(di + o, im, n);
    }
  }
}

__device__ __forceinline__ float coil_div(float acc, float D) { return D == 0.f ? 0.f : __fdiv_rn(acc, D); }

template <bool V4, bool DIM, bool NORM>
__global__ __launch_bounds__(COIL_BLOCK) void coil_combine_kernel(CoilArgs g) {
  for (int64_t i = (int64_t)blockIdx.x * COIL_BLOCK + threadIdx.x; i < g.total; i += (int64_t)gridDim.x * COIL_BLOCK) {
    const int64_t b = i / g.groups, e = (i - b * g.groups) * 4;
    const int n = g.HW - e < 4 ? (int)(g.HW - e) : 4;
    const float* sr = g.s_re + b * g.s_bs + e;
    const float* si = g.s_im + b * g.s_bs + e;
    const float* zr = g.src_re + b * g.src_bs + e;
    const float* zi = g.src_im + b * g.src_bs + e;
    float4 re = make_float4(0.f, 0.f, 0.f, 0.f), im = re, D = re;
#pragma unroll 2
    for (int k = 0; k < g.K; ++k) {
      const int64_t o = (int64_t)k * g.HW;
      const float4 c = coil_ld<V4>(sr + o, n), d = coil_ld<V4>(si + o, n);
      const float4 p = coil_ld<V4>(zr + o, n), q = coil_ld<V4>(zi + o, n);
      re = COIL_EACH(__builtin_fmaf(c.x, p.x, re.x), __builtin_fmaf(c.y, p.y, re.y), __builtin_fmaf(c.z, p.z, re.z),
                     __builtin_fmaf(c.w, p.w, re.w));
      re = COIL_EACH(__builtin_fmaf(d.x, q.x, re.x), __builtin_fmaf(d.y, q.y, re.y), __builtin_fmaf(d.z, q.z, re.z),
                     __builtin_fmaf(d.w, q.w, re.w));
      if (DIM) {
        im = COIL_EACH(__builtin_fmaf(c.x, q.x, im.x), __builtin_fmaf(c.y, q.y, im.y), __builtin_fmaf(c.z, q.z, im.z),
                       __builtin_fmaf(c.w, q.w, im.w));
        im = COIL_EACH(__builtin_fmaf(-d.x, p.x, im.x), __builtin_fmaf(-d.y, p.y, im.y), __builtin_fmaf(-d.z, p.z, im.z),
                       __builtin_fmaf(-d.w, p.w, im.w));
      }
      if (NORM) {
        D = COIL_EACH(__builtin_fmaf(c.x, c.x, D.x), __builtin_fmaf(c.y, c.y, D.y), __builtin_fmaf(c.z, c.z, D.z),
                      __builtin_fmaf(c.w, c.w, D.w));
        D = COIL_EACH(__builtin_fmaf(d.x, d.x, D.x), __builtin_fmaf(d.y, d.y, D.y), __builtin_fmaf(d.z, d.z, D.z),
                      __builtin_fmaf(d.w, d.w, D.w));
      }
    }
    if (NORM) {
      re = COIL_EACH(coil_div(re.x, D.x), coil_div(re.y, D.y), coil_div(re.z, D.z), coil_div(re.w, D.w));
      if (DIM) im = COIL_EACH(coil_div(im.x, D.x), coil_div(im.y, D.y), coil_div(im.z, D.z), coil_div(im.w, D.w));
    }
    coil_st<V4>(g.dst_re + b * g.dst_bs + e, re, n);
    if (DIM) coil_st<V4>(g.dst_im + b * g.dst_bs + e, im, n);
  }
}

#undef COIL_EACH

// The planes p + b * ps + [0, pn) and q + b * qs + [0, qn) floats, b < B, share no float.  Tensors of one stride may interleave
// (the two halves of a (B, 2 K, H, W) tensor); anything else has to lie apart as a whole.
inline bool coil_disjoint(const float* p, int64_t ps, int64_t pn, const float* q, int64_t qs, int64_t qn, int64_t B) {
  const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
  const uint64_t ea = (uint64_t)((B - 1) * ps + pn) * 4, eb = (uint64_t)((B - 1) * qs + qn) * 4;
  if (a + ea <= b || b + eb <= a) return true;
  if (B == 1 || ps != qs || ps <= 0) return false;
  const uint64_t S = (uint64_t)ps * 4;
  const uint64_t r = b >= a ? (b - a) % S : (S - (a - b) % S) % S;  // (q - p) mod S, in bytes
  return r >= (uint64_t)pn * 4 && r + (uint64_t)qn * 4 <= S;
}

inline bool coil_f32(const void* p) { return (((uintptr_t)p) & 3u) == 0; }

// sizes and strides of both entries: every product below fits an int64 with room to spare
inline bool coil_shape_ok(int64_t B, int32_t K, int64_t HW, int64_t dbs, int64_t dn, int64_t abs_, int64_t an, int64_t sbs) {
  if (K < 1 || B < 0 || HW < 0 || HW > ((int64_t)1 << 40) / K) return false;
  if (B > (INT64_MAX >> 4) / (HW > 0 ? (int64_t)K * HW : 1)) return false;
  const int64_t lim = (INT64_MAX >> 3) / (B > 0 ? B : 1);
  if (dbs < 0 || abs_ < 0 || sbs < 0 || dbs > lim || abs_ > lim || sbs > lim) return false;
  if (B > 1 && (dbs < dn || abs_ < an)) return false;  // a tensor's own samples lie apart
  return sbs == 0 || sbs >= (int64_t)K * HW;         // one set of maps for the batch, or one per sample
}

inline bool coil_v4(const CoilArgs& g) {
  return g.HW % 4 == 0 && g.dst_bs % 4 == 0 && g.src_bs % 4 == 0 && g.s_bs % 4 == 0 && AZ_ALIGNED16(g.dst_re) &&
         AZ_ALIGNED16(g.dst_im) && AZ_ALIGNED16(g.src_re) && AZ_ALIGNED16(g.src_im) && AZ_ALIGNED16(g.s_re) && AZ_ALIGNED16(g.s_im);
}

// the 16-byte form where it applies, else the scalar form, on a capped grid
inline void coil_launch(void (*vec)(CoilArgs), void (*scalar)(CoilArgs), const CoilArgs& g, az_stream_t stream) {
  const int64_t blocks = (g.total + COIL_BLOCK - 1) / COIL_BLOCK;
  const dim3 grid((unsigned)(blocks < COIL_GRID ? blocks : COIL_GRID)), block(COIL_BLOCK);
  hipLaunchKernelGGL(coil_v4(g) ? vec : scalar, grid, block, 0, az_s(stream), g);
}

}  // namespace

extern "C" {

int az_op_coil_expand_f32(float* dst_re, float* dst_im, int64_t dst_bstride, const float* x_re, const float* x_im,
                          int64_t x_bstride, const float* s_re, const float* s_im, int64_t s_bstride, int64_t B, int32_t K,
                          int64_t HW, az_stream_t stream) {
  AZ_REQUIRE(coil_shape_ok(B, K, HW, dst_bstride, (int64_t)K * HW, x_bstride, HW, s_bstride), AZ_E_SHAPE);
  if (B == 0 || HW == 0) return AZ_OK;
  AZ_REQUIRE(dst_re && dst_im && x_re && s_re && s_im, AZ_E_NULL);  // (the product with a complex map is complex: dst_im too)
  AZ_REQUIRE(coil_f32(dst_re) && coil_f32(dst_im) && coil_f32(x_re) && coil_f32(x_im) && coil_f32(s_re) && coil_f32(s_im),
             AZ_E_ALIGN);
  const int64_t n = (int64_t)K * HW;
  AZ_REQUIRE(coil_disjoint(dst_re, dst_bstride, n, dst_im, dst_bstride, n, B), AZ_E_SHAPE);
  for (float* d : {dst_re, dst_im}) {  // a workgroup writes where others still read
    AZ_REQUIRE(coil_disjoint(d, dst_bstride, n, x_re, x_bstride, HW, B), AZ_E_SHAPE);
    AZ_REQUIRE(!x_im || coil_disjoint(d, dst_bstride, n, x_im, x_bstride, HW, B), AZ_E_SHAPE);
    AZ_REQUIRE(coil_disjoint(d, dst_bstride, n, s_re, s_bstride, n, B), AZ_E_SHAPE);
    AZ_REQUIRE(coil_disjoint(d, dst_bstride, n, s_im, s_bstride, n, B), AZ_E_SHAPE);
  }
  CoilArgs g;
  g.dst_re = dst_re, g.dst_im = dst_im, g.dst_bs = dst_bstride;
  g.src_re = x_re, g.src_im = x_im, g.src_bs = x_bstride;
  g.s_re = s_re, g.s_im = s_im, g.s_bs = s_bstride;
  g.HW = HW, g.groups = (HW + 3) / 4, g.total = B * g.groups, g.K = K;
  if (x_im) coil_launch(coil_expand_kernel<true, true>, coil_expand_kernel<false, true>, g, stream);
  else coil_launch(coil_expand_kernel<true, false>, coil_expand_kernel<false, false>, g, stream);
  return az_launch_status();
}

int az_op_coil_combine_f32(float* dst_re, float* dst_im, int64_t dst_bstride, const float* z_re, const float* z_im,
                           int64_t z_bstride, const float* s_re, const float* s_im, int64_t s_bstride, int64_t B, int32_t K,
                           int64_t HW, int32_t normalize, az_stream_t stream) {
  AZ_REQUIRE(coil_shape_ok(B, K, HW, dst_bstride, HW, z_bstride, (int64_t)K * HW, s_bstride), AZ_E_SHAPE);
  AZ_REQUIRE(normalize == 0 || normalize == 1, AZ_E_SHAPE);
  if (B == 0 || HW == 0) return AZ_OK;
  AZ_REQUIRE(dst_re && z_re && z_im && s_re && s_im, AZ_E_NULL);  // (coil data is complex: z_im too)
  AZ_REQUIRE(coil_f32(dst_re) && coil_f32(dst_im) && coil_f32(z_re) && coil_f32(z_im) && coil_f32(s_re) && coil_f32(s_im),
             AZ_E_ALIGN);
  const int64_t n = (int64_t)K * HW;
  AZ_REQUIRE(!dst_im || coil_disjoint(dst_re, dst_bstride, HW, dst_im, dst_bstride, HW, B), AZ_E_SHAPE);
  for (float* d : {dst_re, dst_im}) {  // a workgroup writes where others still read
    if (!d) continue;
    AZ_REQUIRE(coil_disjoint(d, dst_bstride, HW, z_re, z_bstride, n, B), AZ_E_SHAPE);
    AZ_REQUIRE(coil_disjoint(d, dst_bstride, HW, z_im, z_bstride, n, B), AZ_E_SHAPE);
    AZ_REQUIRE(coil_disjoint(d, dst_bstride, HW, s_re, s_bstride, n, B), AZ_E_SHAPE);
    AZ_REQUIRE(coil_disjoint(d, dst_bstride, HW, s_im, s_bstride, n, B), AZ_E_SHAPE);
  }
  CoilArgs g;
  g.dst_re = dst_re, g.dst_im = dst_im, g.dst_bs = dst_bstride;
  g.src_re = z_re, g.src_im = z_im, g.src_bs = z_bstride;
  g.s_re = s_re, g.s_im = s_im, g.s_bs = s_bstride;
  g.HW = HW, g.groups = (HW + 3) / 4, g.total = B * g.groups, g.K = K;
  if (dst_im && normalize) coil_launch(coil_combine_kernel<true, true, true>, coil_combine_kernel<false, true, true>, g, stream);
  else if (dst_im) coil_launch(coil_combine_kernel<true, true, false>, coil_combine_kernel<false, true, false>, g, stream);
  else if (normalize) coil_launch(coil_combine_kernel<true, false, true>, coil_combine_kernel<false, false, true>, g, stream);
  else coil_launch(coil_combine_kernel<true, false, false>, coil_combine_kernel<false, false, false>, g, stream);
  return az_launch_status();
}

}  // extern "C"
