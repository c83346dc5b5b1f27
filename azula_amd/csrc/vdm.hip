// The two passes of the v-diffusion backbones (azula/plugins/vdm/_src/*.py) that are not convolutions, norms or attention.
//
// az_fourier_planes_f32 -- the time embedding as constant image planes.  The reference evaluates
//   FourierFeatures (f = 2 pi u w^T, cat[cos f, sin f]), expand_to_planes and torch.cat([input, planes], dim=1)
// per forward; here the planes are channels [c_lo, c_lo + 2 nfeat_half) of the stem convolution's NHWC input, rewritten every
// step from a time on the device.  A thread owns ONE 4-channel chunk of the written range for all the pixels it visits: it
// evaluates its (at most four) features once -- in fp64 from the fp32 time and weights, rounded once -- and then only stores:
// 16 bytes per pixel where the whole chunk lies in the range, single floats on the range's ragged ends (c_lo = 3: channels 3
// and 16..18).  The grid gives every thread >= 8 pixels where there are that many
// (8 x 128 x 128: 43 x 8 workgroups, more than one per CU), so a launch runs one transcendental per ~2 pixels of a 16-feature
// embedding instead of 16 per pixel.
// Bytes: B * HW * 2 nfeat_half * 4 written, nothing read but the time and the nfeat_half weights.
//
// az_upsample_bilinear2x_f32 -- nn.Upsample(scale_factor=2, mode="bilinear", align_corners=False) on NHWC.  With a factor
// of exactly 2 ATen's source coordinate (dst + 0.5) / 2 - 0.5, clamped at 0, lands on
//   dst = 0: (0, 1; weights 1, 0)   dst = 2i > 0: (i - 1, i; 0.25, 0.75)   dst = 2i + 1: (i, min(i + 1, n - 1); 0.75, 0.25)
// per axis, and the value is l0y (l0x v00 + l1x v01) + l1y (l0x v10 + l1x v11) as in ATen.  One thread per output float4:
// four 16-byte loads (three of them shared with the neighbours through L2 / the vector cache), one 16-byte store.
// Bytes: B * H * W * cs * 4 read (compulsory), 4 x that written.
#include "common.h"

#include <math.h>

namespace {

constexpr int FP_THREADS = 256;
constexpr int FP_PIX_PER_THREAD = 8;

__global__ __launch_bounds__(FP_THREADS) void fourier_planes_kernel(float* __restrict__ dst, int64_t HW, int cs, int c_lo, int nh,
                                                                    const float* __restrict__ weight,
                                                                    const float* __restrict__ t_dev, int t_stride, int mode,
                                                                    int q0, int nq) {
  const int b = blockIdx.y;
  const int slots = FP_THREADS / nq;  // pixels in flight per workgroup
  const int q = threadIdx.x % nq, slot = threadIdx.x / nq;
  if (slot >= slots) return;
  // fp64 from the fp32 time on: log(cos^2 / sin^2) is ill conditioned near t = 1 (alpha = cos(t pi / 2) ~ 0.01 at t = 0.9936, where
  // one fp32 rounding of the angle moves u by 2 ang tan(ang) 2^-24 ~ 2e-5 and the feature by 1e-4: torch's own fp32 evaluation
  // misses 16 * 2^-24 * (1 + |f|) there), and a thread evaluates this once for all its pixels
  const double t = (double)t_dev[(int64_t)b * t_stride];
  double u = t;
  if (mode == 1) {  // log(alpha^2 / sigma^2), alpha = cos(t pi / 2), sigma = sin(t pi / 2) (utils.py: t_to_alpha_sigma, alpha_sigma_to_log_snr)
    const double ang = t * 3.14159265358979323846 * 0.5;
    const double al = cos(ang), si = sin(ang);
    u = log((al * al) / (si * si));
  }
  const double tu = 6.283185307179586476925 * u;
  float v[4];
  bool on[4];
  const int c0 = 4 * (q0 + q);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int j = c0 + i - c_lo;
    on[i] = j >= 0 && j < 2 * nh;
    v[i] = 0.f;
    if (on[i]) {
      const double f = tu * (double)weight[j < nh ? j : j - nh];
      v[i] = (float)(j < nh ? cos(f) : sin(f));
    }
  }
  const bool all = on[0] && on[1] && on[2] && on[3];
  float* base = dst + (int64_t)b * HW * cs + c0;
  for (int64_t p = (int64_t)blockIdx.x * slots + slot; p < HW; p += (int64_t)gridDim.x * slots) {
    float* d = base + p * cs;
    if (all) {
      *reinterpret_cast<float4*>(d) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (on[i]) d[i] = v[i];
    }
  }
}

// (first source index, second source index, weight of the second) of output index `o` along an axis of `n` source elements
__device__ __forceinline__ void bilinear2x_taps(int o, int n, int& i0, int& i1, float& l1) {
  if (o == 0) {
    i0 = 0, l1 = 0.f;
  } else if (o & 1) {
    i0 = o >> 1, l1 = 0.25f;
  } else {
    i0 = (o >> 1) - 1, l1 = 0.75f;
  }
  i1 = min(i0 + 1, n - 1);
}

__global__ __launch_bounds__(256) void upsample_bilinear2x_kernel(float* __restrict__ dst, const float* __restrict__ src,
                                                                  int64_t total4, int H, int W, int q) {
  const float4* s4 = reinterpret_cast<const float4*>(src);
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total4; i += (int64_t)gridDim.x * 256) {
    const int c4 = (int)(i % q);
    int64_t r = i / q;
    const int x = (int)(r % (2 * W));
    r /= 2 * W;
    const int y = (int)(r % (2 * H));
    const int64_t b = r / (2 * H);
    int y0, y1, x0, x1;
    float ly, lx;
    bilinear2x_taps(y, H, y0, y1, ly);
    bilinear2x_taps(x, W, x0, x1, lx);
    const float ky = 1.f - ly, kx = 1.f - lx;
    const int64_t r0 = (b * H + y0) * W, r1 = (b * H + y1) * W;
    const float4 a = s4[(r0 + x0) * q + c4], bb = s4[(r0 + x1) * q + c4];
    const float4 c = s4[(r1 + x0) * q + c4], d = s4[(r1 + x1) * q + c4];
    float4 o;
    o.x = ky * (kx * a.x + lx * bb.x) + ly * (kx * c.x + lx * d.x);
    o.y = ky * (kx * a.y + lx * bb.y) + ly * (kx * c.y + lx * d.y);
    o.z = ky * (kx * a.z + lx * bb.z) + ly * (kx * c.z + lx * d.z);
    o.w = ky * (kx * a.w + lx * bb.w) + ly * (kx * c.w + lx * d.w);
    reinterpret_cast<float4*>(dst)[i] = o;
  }
}

}  // namespace

extern "C" {

int az_fourier_planes_f32(float* dst, int64_t B, int64_t HW, int64_t cs, int64_t c_lo, const float* weight,
                          int32_t nfeat_half, const float* t_dev, int64_t t_stride, int32_t mode, az_stream_t stream) {
  AZ_REQUIRE(dst && weight && t_dev, AZ_E_NULL);
  AZ_REQUIRE(B > 0 && B <= 65535 && HW > 0 && cs > 0 && cs % 4 == 0 && cs < (1 << 30) && HW < (1ll << 40), AZ_E_SHAPE);
  AZ_REQUIRE(nfeat_half >= 1 && nfeat_half <= 32 && c_lo >= 0 && c_lo + 2 * (int64_t)nfeat_half <= cs, AZ_E_SHAPE);
  AZ_REQUIRE(t_stride == 0 || t_stride == 1, AZ_E_SHAPE);
  AZ_REQUIRE(mode == 0 || mode == 1, AZ_E_UNSUPPORTED);
  AZ_REQUIRE(AZ_ALIGNED16(dst), AZ_E_ALIGN);
  const int q0 = (int)(c_lo / 4), nq = (int)((c_lo + 2 * nfeat_half + 3) / 4) - q0;  // the 4-channel chunks the range touches (<= 17)
  const int slots = FP_THREADS / nq;
  int64_t gx = (HW + (int64_t)slots * FP_PIX_PER_THREAD - 1) / ((int64_t)slots * FP_PIX_PER_THREAD);
  if (gx > 1024) gx = 1024;
  hipLaunchKernelGGL(fourier_planes_kernel, dim3((unsigned)gx, (unsigned)B), dim3(FP_THREADS), 0, az_s(stream), dst, HW, (int)cs,
                     (int)c_lo, (int)nfeat_half, weight, t_dev, (int)t_stride, (int)mode, q0, nq);
  return az_launch_status();
}

int az_upsample_bilinear2x_f32(float* dst, const float* src, int64_t B, int64_t H, int64_t W, int64_t cs, az_stream_t stream) {
  AZ_REQUIRE(dst && src, AZ_E_NULL);
  AZ_REQUIRE(B > 0 && H > 0 && W > 0 && cs > 0 && cs % 4 == 0, AZ_E_SHAPE);
  // (each factor bounded before the product is formed: H W cs < 2^44 and B < 2^16 keep B H W cs inside int64)
  AZ_REQUIRE(B < (1 << 16) && H < (1 << 29) && W < (1 << 29) && cs < (1 << 30) && H * W < (1ll << 40) / cs, AZ_E_SHAPE);
  AZ_REQUIRE(B * H * W * cs < (1ll << 44), AZ_E_SHAPE);
  AZ_REQUIRE(dst != src, AZ_E_SHAPE);
  AZ_REQUIRE(AZ_ALIGNED16(dst) && AZ_ALIGNED16(src), AZ_E_ALIGN);
  const int64_t total4 = B * 4 * H * W * (cs / 4);
  hipLaunchKernelGGL(upsample_bilinear2x_kernel, dim3(az_stream_grid(total4, 256)), dim3(256), 0, az_s(stream), dst, src, total4,
                     (int)H, (int)W, (int)(cs / 4));
  return az_launch_status();
}

}  // extern "C"
