// RePaint masked resample (azula/guidance/repaint.py:51-61): one streaming pass per RePaint iteration that replaces the
// observed pixels of the DDIM step's x_s by a fresh noisy copy of the observation and re-noises the result back to time t.
//
//   x_s' = mask ? alpha_s * y + sigma_s * n_y : x_s                                (repaint.py:53-57)
//   x_t' = (alpha_t / alpha_s) * x_s' + (alpha_t * sqrt(...)) * n_x                 (repaint.py:59-61)
//
// Separately rounded mul / add in the reference's association order (bit-identical to the torch op sequence on the same
// inputs) and a select, not a blend: a NaN in the unobserved branch never reaches an observed pixel.  HBM-bound like the
// flat transition: 16-byte non-temporal streams, one 32-bit word of mask bytes per float4, grid capped at 16384 workgroups.
#include "common.h"

namespace {

struct RepaintCoef {
  float alpha_s, sigma_s, ratio, kick;  // [alpha_s, sigma_s, alpha_t / alpha_s, alpha_t * sqrt(...)]
};

template <bool XT>
__device__ __forceinline__ void repaint_one(const RepaintCoef& k, float x, float y, bool m, float ny, float nx, float& xs,
                                            float& xt) {
  const float obs = az_add(az_mul(k.alpha_s, y), az_mul(k.sigma_s, ny));
  xs = m ? obs : x;
  if (XT) xt = az_add(az_mul(k.ratio, xs), az_mul(k.kick, nx));
}

__device__ __forceinline__ float4 sel4(uint32_t w, float4 a, float4 b) {  // byte j of w != 0 ? a : b, per lane
  return make_float4((w & 0xFFu) ? a.x : b.x, (w & 0xFF00u) ? a.y : b.y, (w & 0xFF0000u) ? a.z : b.z,
                     (w & 0xFF000000u) ? a.w : b.w);
}

constexpr int RP_UN = 4;  // float4 per thread and stream in flight

template <bool XS, bool XT>
__global__ __launch_bounds__(256) void repaint_kernel(const float* x_s, const float* __restrict__ y,
                                                      const uint8_t* __restrict__ mask, const float* __restrict__ n_y,
                                                      const float* __restrict__ n_x, float* xs_out, float* xt_out,
                                                      const float* __restrict__ coef, int64_t n4, int64_t n) {
  const RepaintCoef k = {coef[0], coef[1], coef[2], coef[3]};
  const uint32_t* mask4 = reinterpret_cast<const uint32_t*>(mask);
  auto one = [&](int64_t i, float4 xv, float4 yv, uint32_t mw, float4 nyv, float4 nxv) {
    float4 obs;
    obs.x = az_add(az_mul(k.alpha_s, yv.x), az_mul(k.sigma_s, nyv.x));
    obs.y = az_add(az_mul(k.alpha_s, yv.y), az_mul(k.sigma_s, nyv.y));
    obs.z = az_add(az_mul(k.alpha_s, yv.z), az_mul(k.sigma_s, nyv.z));
    obs.w = az_add(az_mul(k.alpha_s, yv.w), az_mul(k.sigma_s, nyv.w));
    const float4 s = sel4(mw, obs, xv);
    if (XS) az_st_stream(xs_out + 4 * i, s);
    if (XT) {
      float4 t;
      t.x = az_add(az_mul(k.ratio, s.x), az_mul(k.kick, nxv.x));
      t.y = az_add(az_mul(k.ratio, s.y), az_mul(k.kick, nxv.y));
      t.z = az_add(az_mul(k.ratio, s.z), az_mul(k.kick, nxv.z));
      t.w = az_add(az_mul(k.ratio, s.w), az_mul(k.kick, nxv.w));
      az_st_stream(xt_out + 4 * i, t);
    }
  };
  // the outputs may alias x_s (in-place iteration): all loads of an unrolled group are issued before its first store, and
  // every element is read and written by the same thread only
  const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
  const int64_t span = (int64_t)RP_UN * blockDim.x;
  for (int64_t base = (int64_t)blockIdx.x * span; base + span <= n4; base += (int64_t)gridDim.x * span) {
    const int64_t i = base + threadIdx.x;
    float4 xv[RP_UN], yv[RP_UN], nyv[RP_UN], nxv[RP_UN];
    uint32_t mw[RP_UN];
#pragma unroll
    for (int u = 0; u < RP_UN; ++u) {
      const int64_t q = i + u * blockDim.x;
      xv[u] = az_ld_stream(x_s + 4 * q);
      yv[u] = az_ld_stream(y + 4 * q);
      nyv[u] = az_ld_stream(n_y + 4 * q);
      nxv[u] = XT ? az_ld_stream(n_x + 4 * q) : z4;
      mw[u] = __builtin_nontemporal_load(mask4 + q);
    }
#pragma unroll
    for (int u = 0; u < RP_UN; ++u) one(i + u * blockDim.x, xv[u], yv[u], mw[u], nyv[u], nxv[u]);
  }
  // remainder (fewer than gridDim.x * span float4): plain grid-stride over what is left
  {
    const int64_t done = n4 / span * span;
    for (int64_t i = done + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x)
      one(i, reinterpret_cast<const float4*>(x_s)[i], reinterpret_cast<const float4*>(y)[i], mask4[i],
          reinterpret_cast<const float4*>(n_y)[i], XT ? reinterpret_cast<const float4*>(n_x)[i] : z4);
  }
  // scalar tail (n not a multiple of 4)
  if (blockIdx.x == 0) {
    for (int64_t i = n4 * 4 + threadIdx.x; i < n; i += blockDim.x) {
      float xs, xt;
      repaint_one<XT>(k, x_s[i], y[i], mask[i] != 0, n_y[i], XT ? n_x[i] : 0.f, xs, xt);
      if (XS) xs_out[i] = xs;
      if (XT) xt_out[i] = xt;
    }
  }
}

}  // namespace

extern "C" {

int az_repaint_f32(const AzRepaintArgs* a, az_stream_t stream) {
  AZ_REQUIRE(a && a->x_s && a->y && a->mask && a->n_y && a->coef, AZ_E_NULL);
  AZ_REQUIRE(a->x_s_out || a->x_t_out, AZ_E_NULL);
  AZ_REQUIRE(!a->x_t_out || a->n_x, AZ_E_NULL);
  AZ_REQUIRE(a->n > 0, AZ_E_SHAPE);
  AZ_REQUIRE(AZ_ALIGNED16(a->x_s) && AZ_ALIGNED16(a->y) && AZ_ALIGNED16(a->n_y) && AZ_ALIGNED16(a->x_s_out) &&
                 AZ_ALIGNED16(a->x_t_out) && (!a->x_t_out || AZ_ALIGNED16(a->n_x)) && (((uintptr_t)a->mask) & 3u) == 0,
             AZ_E_ALIGN);
  const int64_t n4 = a->n / 4;
  int64_t g = (n4 + RP_UN * 256 - 1) / (RP_UN * 256);
  const int grid = (int)(g < 1 ? 1 : (g > 16384 ? 16384 : g));
  hipStream_t st = az_s(stream);
#define AZ_RP(XS, XT)                                                                                                  \
  hipLaunchKernelGGL((repaint_kernel<XS, XT>), dim3(grid), dim3(256), 0, st, a->x_s, a->y, a->mask, a->n_y, a->n_x, \
                     a->x_s_out, a->x_t_out, a->coef, n4, a->n)
  if (a->x_s_out && a->x_t_out) AZ_RP(true, true);
  else if (a->x_t_out) AZ_RP(false, true);
  else AZ_RP(true, false);
#undef AZ_RP
  return az_launch_status();
}

}  // extern "C"
