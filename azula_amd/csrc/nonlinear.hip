// The maps of the nonlinear measurement operators (azula_amd/guidance/operators.py: MagnitudeOperator, ClipOperator,
// QuantizeOperator) with their linearisations, and the zero padding of PadOperator.  SPLIT-complex fp32 in az_op_fft2_f32's plane
// convention: sample b of a tensor starts at base + b * bstride floats, the real and the imaginary parts have separate bases, so
// the two halves of one (B, 2 C, H, W) tensor are passed in place.
//
//   az_op_cmag_f32       y = |z| or |z|^2                               12 bytes / element
//   az_op_cmag_vjp_f32   (d_re, d_im) = g (re, im) / |z| or 2 g (re, im)  20
//   az_op_cmag_jvp_f32   t_y = (re t_re + im t_im) / |z| or twice the sum  20
//   az_op_clip_f32       y = min(max(gain x, lo), hi)                      8
//   az_op_clip_jac_f32   d = gain g inside the bounds, else 0             12
//   az_op_quantize_f32   q = rint((clamp(x) - lo) / step) step + lo        8
//   az_op_pad_f32        zero padding of planes, or the crop               4 + 4 per destination float at most
//
// One work item owns 4 consecutive floats of one sample: one aligned float4 per plane where every base, stride and count allows
// it, else (up to) 4 scalars.  Items are a linear int64 range walked with a grid stride by a capped grid.  No atomics and nothing
// shared between items: two launches on the same data give the same bits, and a sample's result does not depend on the other
// samples of the launch.  The linearisations re-read the operating point z or x: the forward kernels save nothing.
//
// Arithmetic of the magnitude.  With h the part of larger and l the part of smaller magnitude, e the exponent that brings |h| into
// [0.5, 1): a = |h| 2^-e, b = |l| 2^-e (exact), s = sqrt(fma(a, a, b b)) with b b rounded on its own, |z| = s 2^e.  s lies in
// [0.5, sqrt 2], so nothing overflows or underflows wherever |z| is a normal fp32 number, and integer Pythagorean pairs below 2^12
// give their hypotenuse exactly at every scale.  |z|^2 is fma(re, re, im im) as written: Inf beyond fp32's range.  A NaN part gives
// NaN.  The unit vector of the linearisations is (re, im) 2^-e / s, one IEEE division each, and exactly (0, 0) at z = 0 (torch's
// sgn convention for abs of a complex tensor); a component below 2^-126 of |z| is a subnormal number with the precision of one.
// The square root is __builtin_sqrtf, correctly rounded under hipcc's default; __fsqrt_rn is the bare 1-ulp instruction here.
#include "common.h"

namespace {

constexpr int NL_BLOCK = 256, NL_GRID = 1024;  // 256 CUs x 4 workgroups, as coil.hip: 16 waves per CU with 16-byte accesses in flight

struct NlArgs {
  float* d0;  // destination planes (d1: the imaginary part, cmag_vjp only)
  float* d1;
  int64_t d_bs;
  const float* a0;  // the operating point: z = (a0, a1), or x = a0
  const float* a1;
  int64_t a_bs;
  const float* b0;  // what the linearisation is applied to: g = b0, or t = (b0, b1)
  const float* b1;
  int64_t b_bs;
  int64_t n, groups, total;  // n floats per sample, groups = ceil(n / 4) items per sample, total = B * groups
  float p0, p1, p2;          // clip: gain, lo, hi; quantize: lo, hi, step
};

// V4: every base and stride is a multiple of 4 floats and n % 4 == 0, so an item is one aligned float4 per plane.  Otherwise the
// item's (up to) 4 floats go one by one; `n` of them lie inside the sample.
template <bool V4>
__device__ __forceinline__ void nl_ld(const float* p, int n, float (&v)[4]) {
  if (V4) {
    const float4 q = *reinterpret_cast<const float4*>(p);
    v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
    return;
  }
  v[0] = p[0];
  v[1] = n > 1 ? p[1] : 0.f;
  v[2] = n > 2 ? p[2] : 0.f;
  v[3] = n > 3 ? p[3] : 0.f;
}
template <bool V4>
__device__ __forceinline__ void nl_st(float* p, const float (&v)[4], int n) {
  if (V4) {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    return;
  }
  p[0] = v[0];
  if (n > 1) p[1] = v[1];
  if (n > 2) p[2] = v[2];
  if (n > 3) p[3] = v[3];
}

// (re, im) 2^-e and s = |z| 2^-e (see the head of the file); e = 0 for z = 0, Inf and NaN, which then pass through sqrt as they are.
struct NlPolar {
  float re, im, s;
  int e;
};
__device__ __forceinline__ NlPolar nl_polar(float re, float im) {
  const float ar = __builtin_fabsf(re), ai = __builtin_fabsf(im);
  const bool first = ar > ai;  // (a NaN part lands in h or in l: both reach the sum)
  const float h = first ? ar : ai, l = first ? ai : ar;
  NlPolar p;
  p.e = __builtin_amdgcn_frexp_expf(h);
  p.re = ldexpf(re, -p.e), p.im = ldexpf(im, -p.e);
  const float a = ldexpf(h, -p.e), b = ldexpf(l, -p.e);
  p.s = __builtin_sqrtf(__builtin_fmaf(a, a, az_mul(b, b)));
  return p;
}

template <bool SQUARED>
struct NlMag {  // d0 = |a| or |a|^2
  static constexpr int NA = 2, NB = 0, ND = 1;
  static __device__ __forceinline__ void run(const NlArgs&, float re, float im, float, float, float& y, float&) {
    if (SQUARED) {
      y = __builtin_fmaf(re, re, az_mul(im, im));
    } else {
      const NlPolar p = nl_polar(re, im);
      y = ldexpf(p.s, p.e);
    }
  }
};

template <bool SQUARED>
struct NlMagVjp {  // (d0, d1) = b0 a / |a| or 2 b0 a
  static constexpr int NA = 2, NB = 1, ND = 2;
  static __device__ __forceinline__ void run(const NlArgs&, float re, float im, float g, float, float& dr, float& di) {
    if (SQUARED) {
      const float g2 = g + g;  // exact
      dr = az_mul(g2, re), di = az_mul(g2, im);
    } else {
      const NlPolar p = nl_polar(re, im);
      const bool zero = re == 0.f && im == 0.f;
      dr = zero ? 0.f : az_mul(g, __fdiv_rn(p.re, p.s));
      di = zero ? 0.f : az_mul(g, __fdiv_rn(p.im, p.s));
    }
  }
};

template <bool SQUARED>
struct NlMagJvp {  // d0 = (a . b) / |a| or 2 (a . b)
  static constexpr int NA = 2, NB = 2, ND = 1;
  static __device__ __forceinline__ void run(const NlArgs&, float re, float im, float tr, float ti, float& ty, float&) {
    if (SQUARED) {
      const float s = __builtin_fmaf(re, tr, az_mul(im, ti));
      ty = s + s;  // exact
    } else {
      const NlPolar p = nl_polar(re, im);
      const bool zero = re == 0.f && im == 0.f;
      ty = zero ? 0.f : __builtin_fmaf(__fdiv_rn(p.re, p.s), tr, az_mul(__fdiv_rn(p.im, p.s), ti));
    }
  }
};

// min(max(v, lo), hi) that keeps a NaN (fminf / fmaxf would return the bound) and the sign of a zero
__device__ __forceinline__ float nl_clamp(float v, float lo, float hi) {
  v = v < lo ? lo : v;
  return v > hi ? hi : v;
}

struct NlClip {  // d0 = clamp(p0 a0, p1, p2)
  static constexpr int NA = 1, NB = 0, ND = 1;
  static __device__ __forceinline__ void run(const NlArgs& g, float x, float, float, float, float& y, float&) {
    y = nl_clamp(az_mul(g.p0, x), g.p1, g.p2);
  }
};

struct NlClipJac {  // d0 = (p1 <= p0 a0 <= p2 ? b0 : 0) p0: torch.clamp's backward, then the product's
  static constexpr int NA = 1, NB = 1, ND = 1;
  static __device__ __forceinline__ void run(const NlArgs& g, float x, float, float v, float, float& d, float&) {
    const float u = az_mul(g.p0, x);
    d = az_mul(u >= g.p1 && u <= g.p2 ? v : 0.f, g.p0);  // (both comparisons are false for a NaN)
  }
};

struct NlQuantize {  // d0 = rint((clamp(a0, p0, p1) - p0) / p2) p2 + p0, every operation rounded once, half to even
  static constexpr int NA = 1, NB = 0, ND = 1;
  static __device__ __forceinline__ void run(const NlArgs& g, float x, float, float, float, float& q, float&) {
    const float u = nl_clamp(x, g.p0, g.p1);
    q = az_add(az_mul(__builtin_rintf(__fdiv_rn(az_sub(u, g.p0), g.p2)), g.p2), g.p0);
  }
};

template <class Op, bool V4>
__global__ __launch_bounds__(NL_BLOCK) void nl_kernel(NlArgs g) {
  for (int64_t i = (int64_t)blockIdx.x * NL_BLOCK + threadIdx.x; i < g.total; i += (int64_t)gridDim.x * NL_BLOCK) {
    const int64_t b = i / g.groups, e = (i - b * g.groups) * 4;
    const int n = g.n - e < 4 ? (int)(g.n - e) : 4;
    float a0[4], a1[4] = {0.f, 0.f, 0.f, 0.f}, b0[4] = {0.f, 0.f, 0.f, 0.f}, b1[4] = {0.f, 0.f, 0.f, 0.f}, d0[4], d1[4];
    nl_ld<V4>(g.a0 + b * g.a_bs + e, n, a0);
    if (Op::NA > 1) nl_ld<V4>(g.a1 + b * g.a_bs + e, n, a1);
    if (Op::NB > 0) nl_ld<V4>(g.b0 + b * g.b_bs + e, n, b0);
    if (Op::NB > 1) nl_ld<V4>(g.b1 + b * g.b_bs + e, n, b1);
#pragma unroll
    for (int k = 0; k < 4; ++k) Op::run(g, a0[k], a1[k], b0[k], b1[k], d0[k], d1[k]);
    nl_st<V4>(g.d0 + b * g.d_bs + e, d0, n);
    if (Op::ND > 1) nl_st<V4>(g.d1 + b * g.d_bs + e, d1, n);
  }
}

// ---- padding -------------------------------------------------------------------------------------------------------------
struct NlPadArgs {
  float* dst;
  const float* src;
  int64_t H, W, Hp, Wp;  // the small and the padded plane
  int64_t top, left;
  int64_t count, total;  // destination floats, total = ceil(count / 4) items
};

// The destination float `o` of the padded tensor (ADJ = false: the source value or 0) or of the cropped one (ADJ = true).
template <bool ADJ>
__device__ __forceinline__ float nl_pad_one(const NlPadArgs& g, int64_t o) {
  if (ADJ) {
    const int64_t c = o % g.W, pr = o / g.W, r = pr % g.H, p = pr / g.H;
    return g.src[(p * g.Hp + r + g.top) * g.Wp + c + g.left];
  }
  const int64_t c = o % g.Wp, pr = o / g.Wp, r = pr % g.Hp, p = pr / g.Hp;
  const int64_t sr = r - g.top, sc = c - g.left;
  return sr >= 0 && sr < g.H && sc >= 0 && sc < g.W ? g.src[(p * g.H + sr) * g.W + sc] : 0.f;
}

// V4: W, Wp and left are multiples of 4 and both tensors 16-byte aligned, so the 4 floats of an item lie in one row, all of them
// inside the image or all outside, and the source's 4 are one aligned float4.
template <bool ADJ, bool V4>
__global__ __launch_bounds__(NL_BLOCK) void nl_pad_kernel(NlPadArgs g) {
  for (int64_t i = (int64_t)blockIdx.x * NL_BLOCK + threadIdx.x; i < g.total; i += (int64_t)gridDim.x * NL_BLOCK) {
    const int64_t o = i * 4;
    if (V4) {
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (ADJ) {
        const int64_t c = o % g.W, pr = o / g.W, r = pr % g.H, p = pr / g.H;
        v = *reinterpret_cast<const float4*>(g.src + (p * g.Hp + r + g.top) * g.Wp + c + g.left);
      } else {
        const int64_t c = o % g.Wp, pr = o / g.Wp, r = pr % g.Hp, p = pr / g.Hp;
        const int64_t sr = r - g.top, sc = c - g.left;
        if (sr >= 0 && sr < g.H && sc >= 0 && sc < g.W) v = *reinterpret_cast<const float4*>(g.src + (p * g.H + sr) * g.W + sc);
      }
      *reinterpret_cast<float4*>(g.dst + o) = v;
    } else {
      const int n = g.count - o < 4 ? (int)(g.count - o) : 4;
      for (int k = 0; k < n; ++k) g.dst[o + k] = nl_pad_one<ADJ>(g, o + k);
    }
  }
}

// ---- validation (host) ----------------------------------------------------------------------------------------------------
// The samples p + b * ps + [0, pn) and q + b * qs + [0, qn) floats, b < B, share no float (coil.hip's rule: tensors of one stride
// may interleave -- the two halves of a (B, 2 C, H, W) tensor -- anything else has to lie apart as a whole).
inline bool nl_disjoint(const float* p, int64_t ps, int64_t pn, const float* q, int64_t qs, int64_t qn, int64_t B) {
  const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
  const uint64_t ea = (uint64_t)((B - 1) * ps + pn) * 4, eb = (uint64_t)((B - 1) * qs + qn) * 4;
  if (a + ea <= b || b + eb <= a) return true;
  if (B == 1 || ps != qs || ps <= 0) return false;
  const uint64_t S = (uint64_t)ps * 4;
  const uint64_t r = b >= a ? (b - a) % S : (S - (a - b) % S) % S;  // (q - p) mod S, in bytes
  return r >= (uint64_t)pn * 4 && r + (uint64_t)qn * 4 <= S;
}

inline bool nl_f32(const void* p) { return (((uintptr_t)p) & 3u) == 0; }

// sizes and strides of the batched entries: every product below fits an int64 with room to spare
inline bool nl_shape_ok(int64_t B, int64_t n, int64_t s0, int64_t s1, int64_t s2) {
  if (B < 0 || n < 0 || n > ((int64_t)1 << 40)) return false;
  if (B > (INT64_MAX >> 4) / (n > 0 ? n : 1)) return false;
  const int64_t lim = (INT64_MAX >> 3) / (B > 0 ? B : 1);
  for (int64_t s : {s0, s1, s2}) {
    if (s < 0 || s > lim) return false;
    if (B > 1 && s < n) return false;  // a tensor's own samples lie apart
  }
  return true;
}

inline bool nl_v4(const NlArgs& g) {
  return g.n % 4 == 0 && g.d_bs % 4 == 0 && g.a_bs % 4 == 0 && g.b_bs % 4 == 0 && AZ_ALIGNED16(g.d0) && AZ_ALIGNED16(g.d1) &&
         AZ_ALIGNED16(g.a0) && AZ_ALIGNED16(g.a1) && AZ_ALIGNED16(g.b0) && AZ_ALIGNED16(g.b1);
}

inline dim3 nl_grid(int64_t total) {
  const int64_t blocks = (total + NL_BLOCK - 1) / NL_BLOCK;
  return dim3((unsigned)(blocks < NL_GRID ? blocks : NL_GRID));
}

// Checks shared by the elementwise entries, then the launch: the 16-byte form where it applies, else the scalar form.  `B`
// samples of `n` floats; unused planes are NULL with stride 0.
template <class Op>
int nl_run(NlArgs g, int64_t B, az_stream_t stream) {
  AZ_REQUIRE(nl_shape_ok(B, g.n, g.d_bs, Op::NA ? g.a_bs : g.n, Op::NB ? g.b_bs : g.n), AZ_E_SHAPE);
  if (B == 0 || g.n == 0) return AZ_OK;
  AZ_REQUIRE(g.d0 && g.a0 && (Op::ND < 2 || g.d1) && (Op::NA < 2 || g.a1) && (Op::NB < 1 || g.b0) && (Op::NB < 2 || g.b1), AZ_E_NULL);
  AZ_REQUIRE(nl_f32(g.d0) && nl_f32(g.d1) && nl_f32(g.a0) && nl_f32(g.a1) && nl_f32(g.b0) && nl_f32(g.b1), AZ_E_ALIGN);
  AZ_REQUIRE(!g.d1 || nl_disjoint(g.d0, g.d_bs, g.n, g.d1, g.d_bs, g.n, B), AZ_E_SHAPE);
  for (float* d : {g.d0, g.d1}) {  // a workgroup writes where others still read
    if (!d) continue;
    for (const float* s : {g.a0, g.a1}) AZ_REQUIRE(!s || nl_disjoint(d, g.d_bs, g.n, s, g.a_bs, g.n, B), AZ_E_SHAPE);
    for (const float* s : {g.b0, g.b1}) AZ_REQUIRE(!s || nl_disjoint(d, g.d_bs, g.n, s, g.b_bs, g.n, B), AZ_E_SHAPE);
  }
  g.groups = (g.n + 3) / 4, g.total = B * g.groups;
  void (*vec)(NlArgs) = nl_kernel<Op, true>, (*scalar)(NlArgs) = nl_kernel<Op, false>;
  hipLaunchKernelGGL(nl_v4(g) ? vec : scalar, nl_grid(g.total), dim3(NL_BLOCK), 0, az_s(stream), g);
  return az_launch_status();
}

inline NlArgs nl_args(float* d0, float* d1, int64_t d_bs, const float* a0, const float* a1, int64_t a_bs, const float* b0,
                      const float* b1, int64_t b_bs, int64_t n) {
  NlArgs g;
  g.d0 = d0, g.d1 = d1, g.d_bs = d_bs, g.a0 = a0, g.a1 = a1, g.a_bs = a_bs, g.b0 = b0, g.b1 = b1, g.b_bs = b_bs;
  g.n = n, g.groups = 0, g.total = 0, g.p0 = g.p1 = g.p2 = 0.f;
  return g;
}

inline bool nl_finite(float v) { return v - v == 0.f; }

}  // namespace

extern "C" {

int az_op_nonlinear_trip(int64_t* floats) {
  AZ_REQUIRE(floats, AZ_E_NULL);
  *floats = (int64_t)NL_GRID * NL_BLOCK * 4;
  return AZ_OK;
}

int az_op_cmag_f32(float* y, int64_t y_bstride, const float* z_re, const float* z_im, int64_t z_bstride, int64_t B, int64_t n,
                   int32_t squared, az_stream_t stream) {
  AZ_REQUIRE(squared == 0 || squared == 1, AZ_E_SHAPE);
  const NlArgs g = nl_args(y, nullptr, y_bstride, z_re, z_im, z_bstride, nullptr, nullptr, 0, n);
  return squared ? nl_run<NlMag<true>>(g, B, stream) : nl_run<NlMag<false>>(g, B, stream);
}

int az_op_cmag_vjp_f32(float* d_re, float* d_im, int64_t d_bstride, const float* g, int64_t g_bstride, const float* z_re,
                       const float* z_im, int64_t z_bstride, int64_t B, int64_t n, int32_t squared, az_stream_t stream) {
  AZ_REQUIRE(squared == 0 || squared == 1, AZ_E_SHAPE);
  const NlArgs a = nl_args(d_re, d_im, d_bstride, z_re, z_im, z_bstride, g, nullptr, g_bstride, n);
  return squared ? nl_run<NlMagVjp<true>>(a, B, stream) : nl_run<NlMagVjp<false>>(a, B, stream);
}

int az_op_cmag_jvp_f32(float* t_y, int64_t y_bstride, const float* t_re, const float* t_im, int64_t t_bstride, const float* z_re,
                       const float* z_im, int64_t z_bstride, int64_t B, int64_t n, int32_t squared, az_stream_t stream) {
  AZ_REQUIRE(squared == 0 || squared == 1, AZ_E_SHAPE);
  const NlArgs a = nl_args(t_y, nullptr, y_bstride, z_re, z_im, z_bstride, t_re, t_im, t_bstride, n);
  return squared ? nl_run<NlMagJvp<true>>(a, B, stream) : nl_run<NlMagJvp<false>>(a, B, stream);
}

int az_op_clip_f32(float* y, const float* x, int64_t n, float gain, float lo, float hi, az_stream_t stream) {
  AZ_REQUIRE(nl_finite(gain) && nl_finite(lo) && nl_finite(hi) && lo < hi, AZ_E_SHAPE);
  NlArgs g = nl_args(y, nullptr, 0, x, nullptr, 0, nullptr, nullptr, 0, n);
  g.p0 = gain, g.p1 = lo, g.p2 = hi;
  return nl_run<NlClip>(g, 1, stream);
}

int az_op_clip_jac_f32(float* d, const float* g, const float* x, int64_t n, float gain, float lo, float hi, az_stream_t stream) {
  AZ_REQUIRE(nl_finite(gain) && nl_finite(lo) && nl_finite(hi) && lo < hi, AZ_E_SHAPE);
  NlArgs a = nl_args(d, nullptr, 0, x, nullptr, 0, g, nullptr, 0, n);
  a.p0 = gain, a.p1 = lo, a.p2 = hi;
  return nl_run<NlClipJac>(a, 1, stream);
}

int az_op_quantize_f32(float* q, const float* x, int64_t n, float lo, float hi, float step, az_stream_t stream) {
  AZ_REQUIRE(nl_finite(lo) && nl_finite(hi) && nl_finite(step) && lo < hi && step > 0.f, AZ_E_SHAPE);
  NlArgs g = nl_args(q, nullptr, 0, x, nullptr, 0, nullptr, nullptr, 0, n);
  g.p0 = lo, g.p1 = hi, g.p2 = step;
  return nl_run<NlQuantize>(g, 1, stream);
}

int az_op_pad_f32(float* dst, const float* src, int64_t planes, int64_t H, int64_t W, int32_t top, int32_t bottom, int32_t left,
                  int32_t right, int32_t adjoint, az_stream_t stream) {
  constexpr int64_t LIM = (int64_t)1 << 20;  // per side and per pad: planes * Hp * Wp stays far inside an int64
  AZ_REQUIRE(planes >= 0 && H >= 0 && W >= 0 && H <= LIM && W <= LIM && planes <= ((int64_t)1 << 40), AZ_E_SHAPE);
  AZ_REQUIRE(top >= 0 && bottom >= 0 && left >= 0 && right >= 0 && top <= LIM && bottom <= LIM && left <= LIM && right <= LIM,
             AZ_E_SHAPE);
  AZ_REQUIRE(adjoint == 0 || adjoint == 1, AZ_E_SHAPE);
  NlPadArgs g;
  g.dst = dst, g.src = src, g.H = H, g.W = W, g.Hp = H + top + bottom, g.Wp = W + left + right, g.top = top, g.left = left;
  const int64_t small = planes * H * W, big = planes * g.Hp * g.Wp;
  g.count = adjoint ? small : big;
  if (g.count == 0) return AZ_OK;
  const int64_t from = adjoint ? big : small;  // (0 for the padding of empty planes: all zeros, nothing is read)
  AZ_REQUIRE(dst && (src || from == 0), AZ_E_NULL);
  AZ_REQUIRE(nl_f32(dst) && nl_f32(src), AZ_E_ALIGN);
  AZ_REQUIRE(from == 0 || nl_disjoint(dst, 0, g.count, src, 0, from, 1), AZ_E_SHAPE);
  g.total = (g.count + 3) / 4;
  const bool v4 = W % 4 == 0 && g.Wp % 4 == 0 && left % 4 == 0 && AZ_ALIGNED16(dst) && AZ_ALIGNED16(src);
  void (*pad[2][2])(NlPadArgs) = {{nl_pad_kernel<false, false>, nl_pad_kernel<false, true>},
                                  {nl_pad_kernel<true, false>, nl_pad_kernel<true, true>}};
  hipLaunchKernelGGL(pad[adjoint][v4], nl_grid(g.total), dim3(NL_BLOCK), 0, az_s(stream), g);
  return az_launch_status();
}

}  // extern "C"
