// SPD-mix downsamplers DMConv / DMMConv / DMMConv2 (models/common.py:1460-1475 SM / MP, 1508-1547): the SM fold
// (2 x 2 pixels into channels) inside the BatchNorm / activation passes of the stride-1 conv that feeds it, the 2 x 2
// stride-2 max pool of the second branch, and DMMConv2's front end that reads x once for both SM(x) and MP(x).
//
// All kernels are streaming passes over NHWC rows, bandwidth-bound: 16-byte loads and stores (C % 8 == 0 in bf16,
// C % 4 == 0 in fp32, 16-byte aligned bases and pixel strides), fp32 arithmetic, one rounding to storage per output
// element, no atomics.  Every tensor has its own pixel stride, so the SM side may be a channel slice of a concat buffer.
// Anything else returns hipErrorInvalidValue and launches nothing.
//
// SM layout (cat(x[::2, ::2], x[1::2, ::2], x[::2, 1::2], x[1::2, 1::2]), = space_to_depth in eltwise.hip): the
// full-resolution pixel (n, h, w) with K channels is the K-channel block q = (h & 1) + 2 * (w & 1) of the
// half-resolution pixel (n, h / 2, w / 2).  H and W are even.
//
// The three BN passes are bn.hip's bn_act_fwd_vec / bn_bwd_reduce_vec / bn_bwd_apply_vec with the SM-side address
// replaced: same thread mapping (RowMap), same grids, same row order, the per-channel expressions of common.h's
// act_fwd_n / act_grad_n, so each gives the bits of the plain pass composed with dmy_space_to_depth.
#include "launch.h"

namespace {

// bn.hip's thread mapping: a block of 256 threads covers RB rows x CV channel-vectors, a thread keeps one
// channel-vector for the whole launch; rows are grid-strided
struct RowMap {
  int cv, rr, RB, CV;
  DEV RowMap(int C, int VW) {
    CV = C / VW;
    RB = 256 / CV;
    cv = threadIdx.x % CV;
    rr = threadIdx.x / CV;
  }
  DEV bool active() const { return rr < RB; }
};

// full-resolution NHWC pixel m -> its half-resolution pixel and K-channel block q.  32-bit divisions whenever the
// pixel count fits (a 64-bit division is a long software sequence)
DEV long sm_pixel(long m, int H, int W, bool small, int& q) {
  int w, h, b;
  if (small) {
    const unsigned u = (unsigned)m, t = u / (unsigned)W;
    w = (int)(u - t * (unsigned)W);
    b = (int)(t / (unsigned)H);
    h = (int)(t - (unsigned)b * (unsigned)H);
  } else {
    w = (int)(m % W);
    h = (int)((m / W) % H);
    b = (int)(m / ((long)W * H));
  }
  q = (h & 1) + 2 * (w & 1);
  return ((long)b * (H >> 1) + (h >> 1)) * (W >> 1) + (w >> 1);
}

// -------- y_sm = act(z * scale + shift): rows walked from the end, as dmy_bn_act_fwd (bn.hip kRevAct)
template <typename T>
__global__ void __launch_bounds__(256) bn_act_s2d_fwd_kernel(const T* __restrict__ z, long zps,
                                                             const float* __restrict__ scale,
                                                             const float* __restrict__ shift, int act,
                                                             T* __restrict__ y, long yps, int N, int H, int W, int K) {
  constexpr int VW = Traits<T>::VW;
  RowMap rm(K, VW);
  if (!rm.active()) return;
  const int c0 = rm.cv * VW;
  float sc[VW], sh[VW];
  ldf<VW>(scale + c0, sc);
  ldf<VW>(shift + c0, sh);
  const long M = (long)N * H * W, S = (long)gridDim.x * rm.RB;
  const bool small = M < (1L << 31);
  for (long i = (long)blockIdx.x * rm.RB + rm.rr; i < M; i += S) {
    const long m = M - 1 - i;
    int q;
    const long op = sm_pixel(m, H, W, small, q);
    float f[VW];
    unpack<T>(*reinterpret_cast<const uint4*>(z + m * zps + c0), f);
#pragma unroll
    for (int j = 0; j < VW; ++j) f[j] = f[j] * sc[j] + sh[j];
    act_fwd_n<VW>(act, f);
    *reinterpret_cast<uint4*>(y + op * yps + (long)q * K + c0) = pack<T>(f);
  }
}

// -------- backward reduce: per channel sum(du), sum(du * xhat), du = dy_sm * act'(u); one partial row per block, rows
// in increasing order (deterministic)
template <typename T>
__global__ void __launch_bounds__(256) bn_bwd_reduce_s2d_kernel(const T* __restrict__ z, long zps,
                                                                const T* __restrict__ dy, long dps,
                                                                const float* __restrict__ scale,
                                                                const float* __restrict__ shift,
                                                                const float* __restrict__ mean,
                                                                const float* __restrict__ invstd, int act, int N, int H,
                                                                int W, int K, float* __restrict__ pdb,
                                                                float* __restrict__ pdg) {
  constexpr int VW = Traits<T>::VW;
  __shared__ float red[2][256 * VW];
  RowMap rm(K, VW);
  const int c0 = rm.cv * VW;
  float a[VW], b[VW];
#pragma unroll
  for (int j = 0; j < VW; ++j) { a[j] = 0.f; b[j] = 0.f; }
  if (rm.active()) {
    float sc[VW], sh[VW], mu[VW], is[VW];
    ldf<VW>(scale + c0, sc);
    ldf<VW>(shift + c0, sh);
    ldf<VW>(mean + c0, mu);
    ldf<VW>(invstd + c0, is);
    const long M = (long)N * H * W, S = (long)gridDim.x * rm.RB;
    const bool small = M < (1L << 31);
    for (long m = (long)blockIdx.x * rm.RB + rm.rr; m < M; m += S) {
      int q;
      const long op = sm_pixel(m, H, W, small, q);
      const uint4 zv = *reinterpret_cast<const uint4*>(z + m * zps + c0);
      const uint4 gv = *reinterpret_cast<const uint4*>(dy + op * dps + (long)q * K + c0);
      float zf[VW], gf[VW], ag[VW];
      unpack<T>(zv, zf);
      unpack<T>(gv, gf);
#pragma unroll
      for (int j = 0; j < VW; ++j) ag[j] = zf[j] * sc[j] + sh[j];
      act_grad_n<VW>(act, ag);
#pragma unroll
      for (int j = 0; j < VW; ++j) {
        const float du = gf[j] * ag[j];
        a[j] += du;
        b[j] += du * (zf[j] - mu[j]) * is[j];
      }
    }
  }
#pragma unroll
  for (int j = 0; j < VW; ++j) {
    red[0][threadIdx.x * VW + j] = a[j];
    red[1][threadIdx.x * VW + j] = b[j];
  }
  __syncthreads();
  // one thread per channel sums the RB row groups in order
  for (int c = threadIdx.x; c < K; c += blockDim.x) {
    const int cv = c / VW, j = c % VW;
    float s1 = 0.f, s2 = 0.f;
    for (int r = 0; r < rm.RB; ++r) {
      const int t = r * rm.CV + cv;
      s1 += red[0][t * VW + j];
      s2 += red[1][t * VW + j];
    }
    pdb[(long)blockIdx.x * K + c] = s1;
    pdg[(long)blockIdx.x * K + c] = s2;
  }
}

// -------- dz = ca * du + cb + cc * xhat with dy read through the SM mapping; rows from the end (bn.hip kRevApply)
template <typename T>
__global__ void __launch_bounds__(256) bn_bwd_apply_s2d_kernel(const T* __restrict__ z, long zps,
                                                               const T* __restrict__ dy, long dps,
                                                               const float* __restrict__ scale,
                                                               const float* __restrict__ shift,
                                                               const float* __restrict__ mean,
                                                               const float* __restrict__ invstd, int act,
                                                               const float* __restrict__ ca, const float* __restrict__ cb,
                                                               const float* __restrict__ cc, T* __restrict__ dz,
                                                               long dzps, int N, int H, int W, int K) {
  constexpr int VW = Traits<T>::VW;
  RowMap rm(K, VW);
  if (!rm.active()) return;
  const int c0 = rm.cv * VW;
  float sc[VW], sh[VW], k1[VW], k0[VW], k2[VW], t0[VW], t1[VW];
  ldf<VW>(scale + c0, sc);
  ldf<VW>(shift + c0, sh);
  ldf<VW>(ca + c0, k1);
  ldf<VW>(cc + c0, k2);
  ldf<VW>(invstd + c0, t0);
  ldf<VW>(cb + c0, k0);
  ldf<VW>(mean + c0, t1);
#pragma unroll
  for (int j = 0; j < VW; ++j) {
    // dz = ca*du + cb + cc*(z - mean)*invstd = ca*du + k0 + k2*z
    k2[j] = k2[j] * t0[j];
    k0[j] = k0[j] - k2[j] * t1[j];
  }
  const long M = (long)N * H * W, S = (long)gridDim.x * rm.RB;
  const bool small = M < (1L << 31);
  for (long i = (long)blockIdx.x * rm.RB + rm.rr; i < M; i += S) {
    const long m = M - 1 - i;
    int q;
    const long op = sm_pixel(m, H, W, small, q);
    const uint4 zv = *reinterpret_cast<const uint4*>(z + m * zps + c0);
    const uint4 gv = *reinterpret_cast<const uint4*>(dy + op * dps + (long)q * K + c0);
    float zf[VW], gf[VW], o[VW];
    unpack<T>(zv, zf);
    unpack<T>(gv, gf);
#pragma unroll
    for (int j = 0; j < VW; ++j) o[j] = zf[j] * sc[j] + sh[j];
    act_grad_n<VW>(act, o);
#pragma unroll
    for (int j = 0; j < VW; ++j) o[j] = k1[j] * (gf[j] * o[j]) + k0[j] + k2[j] * zf[j];
    *reinterpret_cast<uint4*>(dz + m * dzps + c0) = pack<T>(o);
  }
}

// -------- nn.MaxPool2d(2, 2) and DMMConv2's front end
// a vector index over [N][PH][PW][CV] -> (pixel index, first channel); 32-bit divisions whenever it fits
DEV void vec_pixel(long i, int PH, int PW, int CV, int VW, int& b, int& h, int& w, int& c) {
  if ((unsigned long)i < 0xFFFFFFFFul) {
    const unsigned u = (unsigned)i, t0 = u / (unsigned)CV, t1 = t0 / (unsigned)PW;
    c = (int)(u - t0 * (unsigned)CV) * VW;
    w = (int)(t0 - t1 * (unsigned)PW);
    b = (int)(t1 / (unsigned)PH);
    h = (int)(t1 - (unsigned)b * (unsigned)PH);
    return;
  }
  c = (int)(i % CV) * VW;
  long t = i / CV;
  w = (int)(t % PW);
  t /= PW;
  h = (int)(t % PH);
  b = (int)(t / PH);
}

template <int VW> DEV void st_arg(unsigned char* p, const int* bi) {
  unsigned char a[VW];
#pragma unroll
  for (int j = 0; j < VW; ++j) a[j] = (unsigned char)bi[j];
  if constexpr (VW == 8) *reinterpret_cast<uint2*>(p) = *reinterpret_cast<const uint2*>(a);
  else *reinterpret_cast<uint32_t*>(p) = *reinterpret_cast<const uint32_t*>(a);
}
template <int VW> DEV void ld_arg(const unsigned char* p, int* bi) {
  unsigned char a[VW];
  if constexpr (VW == 8) *reinterpret_cast<uint2*>(a) = *reinterpret_cast<const uint2*>(p);
  else *reinterpret_cast<uint32_t*>(a) = *reinterpret_cast<const uint32_t*>(p);
#pragma unroll
  for (int j = 0; j < VW; ++j) bi[j] = a[j];
}

// One thread per 16-byte vector of the pooled map: the window's four vectors are loaded back to back, the maximum
// follows ATen's max_pool2d rule (scan (0,0), (0,1), (1,0), (1,1); update when v > best || isnan(v), from -inf), and
// the window offset dh * 2 + dw of the winner goes to arg [N * OH * OW][C].  SPLIT: the four vectors are also stored
// as the K-channel blocks dh + 2 * dw of the SM pixel (H, W even), so x is read once for both branches.
template <typename T, bool SPLIT>
__global__ void __launch_bounds__(256) maxpool2_fwd_kernel(const T* __restrict__ x, long xps, T* __restrict__ y, long yps,
                                                           unsigned char* __restrict__ arg, T* __restrict__ sm,
                                                           long smps, int N, int H, int W, int C) {
  constexpr int VW = Traits<T>::VW;
  const int OH = H / 2, OW = W / 2, CV = C / VW;
  const long total = (long)N * OH * OW * CV;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    int b, oh, ow, c;
    vec_pixel(i, OH, OW, CV, VW, b, oh, ow, c);
    const long ip = ((long)b * H + 2 * oh) * W + 2 * ow, op = ((long)b * OH + oh) * OW + ow;
    uint4 v[4];
#pragma unroll
    for (int t = 0; t < 4; ++t)
      v[t] = *reinterpret_cast<const uint4*>(x + (ip + (long)(t >> 1) * W + (t & 1)) * xps + c);
    float best[VW];
    int bi[VW];
#pragma unroll
    for (int j = 0; j < VW; ++j) { best[j] = -INFINITY; bi[j] = 0; }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      float f[VW];
      unpack<T>(v[t], f);
#pragma unroll
      for (int j = 0; j < VW; ++j) {
        // bitwise (not short-circuit) so the selects stay branch-free
        const unsigned up = (unsigned)(f[j] > best[j]) | (unsigned)__builtin_isnan(f[j]);
        best[j] = up ? f[j] : best[j];
        bi[j] = up ? t : bi[j];
      }
      if constexpr (SPLIT) {  // t = dh * 2 + dw -> block dh + 2 * dw
        *reinterpret_cast<uint4*>(sm + op * smps + (long)((t >> 1) + 2 * (t & 1)) * C + c) = v[t];
      }
    }
    *reinterpret_cast<uint4*>(y + op * yps + c) = pack<T>(best);
    st_arg<VW>(arg + op * C + c, bi);
  }
}

// Backward as a gather, one thread per 16-byte vector of dx: the input pixel (h, w) belongs to the one window
// (h / 2, w / 2) (to none in the last row / column of an odd map) and takes its gradient when arg names it.  SPLIT:
// dx = SM^-1(dsm) + that gradient, summed in fp32 and rounded once.  accumulate (not SPLIT): dx += for a GradSink.
template <typename T, bool SPLIT>
__global__ void __launch_bounds__(256) maxpool2_bwd_kernel(const T* __restrict__ dy, long dps,
                                                           const unsigned char* __restrict__ arg,
                                                           const T* __restrict__ dsm, long dsmps, T* __restrict__ dx,
                                                           long dxps, int accumulate, int N, int H, int W, int C) {
  constexpr int VW = Traits<T>::VW;
  const int OH = H / 2, OW = W / 2, CV = C / VW;
  const long total = (long)N * H * W * CV;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    int b, h, w, c;
    vec_pixel(i, H, W, CV, VW, b, h, w, c);
    const int oh = h >> 1, ow = w >> 1, t = (h & 1) * 2 + (w & 1);
    const bool in = oh < OH && ow < OW;
    const long op = ((long)b * OH + oh) * OW + ow;
    float g[VW];
#pragma unroll
    for (int j = 0; j < VW; ++j) g[j] = 0.f;
    if (in) {
      int bi[VW];
      ld_arg<VW>(arg + op * C + c, bi);
      float f[VW];
      unpack<T>(*reinterpret_cast<const uint4*>(dy + op * dps + c), f);
#pragma unroll
      for (int j = 0; j < VW; ++j) g[j] = bi[j] == t ? f[j] : 0.f;
    }
    T* o = dx + (((long)b * H + h) * W + w) * dxps + c;
    if constexpr (SPLIT) {
      float f[VW];
      unpack<T>(*reinterpret_cast<const uint4*>(dsm + op * dsmps + (long)((h & 1) + 2 * (w & 1)) * C + c), f);
#pragma unroll
      for (int j = 0; j < VW; ++j) g[j] += f[j];
    } else if (accumulate) {
      float f[VW];
      unpack<T>(*reinterpret_cast<const uint4*>(o), f);
#pragma unroll
      for (int j = 0; j < VW; ++j) g[j] += f[j];
    }
    *reinterpret_cast<uint4*>(o) = pack<T>(g);
  }
}

// Besides the vector contract, at every call site: a row is 1..256 vectors (RowMap) and fits its stride; the SM side
// holds 4 K channels per pixel; the argmax rows are stored 8 bytes at a time.  The grids are those of bn.hip's passes.

}  // namespace

DMY_API int dmy_bn_act_s2d_fwd(int dtype, const void* z, long zps, const float* scale, const float* shift, int act,
                               void* y, long yps, int N, int H, int W, int K, void* stream) {
  const int VW = vec_width(dtype);
  if (N < 1 || H < 2 || W < 2 || ((H | W) & 1) || K < VW || K / VW > 256 || !vec_ok(VW, K, {zps, yps}, {z, y}) ||
      zps < K || yps < 4L * K || !scale || !shift)
    return kInvalid;
  return by_dtype(dtype, kInvalid, [&](auto tag) {
    using T = typename decltype(tag)::type;
    return launch(bn_act_s2d_fwd_kernel<T>, row_grid((long)N * H * W, K, VW, kEwCap), stream, z, zps, scale, shift, act,
        y, yps, N, H, W, K);
  });
}

DMY_API int dmy_bn_bwd_reduce_s2d_rows(int dtype, long M, int K) {
  const int VW = vec_width(dtype);
  if (M < 1 || K < VW || K % VW || K / VW > 256) return 0;
  return row_grid(M, K, VW, kRedCap);
}

DMY_API int dmy_bn_bwd_reduce_s2d(int dtype, const void* z, long zps, const void* dy, long dps, const float* scale,
                                  const float* shift, const float* mean, const float* invstd, int act, int N, int H,
                                  int W, int K, float* pdb, float* pdg, void* stream) {
  const int VW = vec_width(dtype);
  if (N < 1 || H < 2 || W < 2 || ((H | W) & 1) || K < VW || K / VW > 256 || !vec_ok(VW, K, {zps, dps}, {z, dy}) ||
      zps < K || dps < 4L * K || !scale || !shift || !mean || !invstd || !pdb || !pdg)
    return kInvalid;
  return by_dtype(dtype, kInvalid, [&](auto tag) {
    using T = typename decltype(tag)::type;
    return launch(bn_bwd_reduce_s2d_kernel<T>, dmy_bn_bwd_reduce_s2d_rows(dtype, (long)N * H * W, K), stream, z, zps,
        dy, dps, scale, shift, mean, invstd, act, N, H, W, K, pdb, pdg);
  });
}

DMY_API int dmy_bn_bwd_apply_s2d(int dtype, const void* z, long zps, const void* dy, long dps, const float* scale,
                                 const float* shift, const float* mean, const float* invstd, int act, const float* ca,
                                 const float* cb, const float* cc, void* dz, long dzps, int N, int H, int W, int K,
                                 void* stream) {
  const int VW = vec_width(dtype);
  if (N < 1 || H < 2 || W < 2 || ((H | W) & 1) || K < VW || K / VW > 256 ||
      !vec_ok(VW, K, {zps, dzps, dps}, {z, dy, dz}) || !rows_fit(K, {zps, dzps}) || dps < 4L * K || !scale || !shift ||
      !mean || !invstd || !ca || !cb || !cc)
    return kInvalid;
  return by_dtype(dtype, kInvalid, [&](auto tag) {
    using T = typename decltype(tag)::type;
    return launch(bn_bwd_apply_s2d_kernel<T>, row_grid((long)N * H * W, K, VW, kEwCap), stream, z, zps, dy, dps, scale,
        shift, mean, invstd, act, ca, cb, cc, dz, dzps, N, H, W, K);
  });
}

DMY_API int dmy_maxpool2_fwd(int dtype, const void* x, long xps, void* y, long yps, unsigned char* argmax, int N, int H,
                             int W, int C, void* stream) {
  const int VW = vec_width(dtype);
  if (N < 1 || H < 2 || W < 2 || C < VW || C / VW > 256 || !vec_ok(VW, C, {xps, yps}, {x, y}) ||
      !rows_fit(C, {xps, yps}) || !argmax || ((uintptr_t)argmax & 7))
    return kInvalid;
  return by_dtype(dtype, kInvalid, [&](auto tag) {
    using T = typename decltype(tag)::type;
    return launch(maxpool2_fwd_kernel<T, false>, vgrid((long)N * (H / 2) * (W / 2) * (C / VW)), stream, x, xps, y, yps,
        argmax, nullptr, 0, N, H, W, C);
  });
}

DMY_API int dmy_maxpool2_bwd(int dtype, const void* dy, long dps, const unsigned char* argmax, void* dx, long dxps,
                             int accumulate, int N, int H, int W, int C, void* stream) {
  const int VW = vec_width(dtype);
  if (N < 1 || H < 2 || W < 2 || C < VW || C / VW > 256 || !vec_ok(VW, C, {dps, dxps}, {dy, dx}) ||
      !rows_fit(C, {dps, dxps}) || !argmax || ((uintptr_t)argmax & 7))
    return kInvalid;
  return by_dtype(dtype, kInvalid, [&](auto tag) {
    using T = typename decltype(tag)::type;
    return launch(maxpool2_bwd_kernel<T, false>, vgrid((long)N * H * W * (C / VW)), stream, dy, dps, argmax, nullptr, 0,
        dx, dxps, accumulate, N, H, W, C);
  });
}

DMY_API int dmy_spd_split_fwd(int dtype, const void* x, long xps, void* sm, long smps, void* mp, long mpps,
                              unsigned char* argmax, int N, int H, int W, int C, void* stream) {
  const int VW = vec_width(dtype);
  if (N < 1 || H < 2 || W < 2 || ((H | W) & 1) || C < VW || C / VW > 256 ||
      !vec_ok(VW, C, {xps, mpps, smps}, {x, sm, mp}) || !rows_fit(C, {xps, mpps}) || smps < 4L * C || !argmax ||
      ((uintptr_t)argmax & 7))
    return kInvalid;
  return by_dtype(dtype, kInvalid, [&](auto tag) {
    using T = typename decltype(tag)::type;
    return launch(maxpool2_fwd_kernel<T, true>, vgrid((long)N * (H / 2) * (W / 2) * (C / VW)), stream, x, xps, mp, mpps,
        argmax, sm, smps, N, H, W, C);
  });
}

DMY_API int dmy_spd_split_bwd(int dtype, const void* dsm, long dsmps, const void* dmp, long dmpps,
                              const unsigned char* argmax, void* dx, long dxps, int N, int H, int W, int C,
                              void* stream) {
  const int VW = vec_width(dtype);
  if (N < 1 || H < 2 || W < 2 || ((H | W) & 1) || C < VW || C / VW > 256 ||
      !vec_ok(VW, C, {dmpps, dxps, dsmps}, {dsm, dmp, dx}) || !rows_fit(C, {dmpps, dxps}) || dsmps < 4L * C || !argmax ||
      ((uintptr_t)argmax & 7))
    return kInvalid;
  return by_dtype(dtype, kInvalid, [&](auto tag) {
    using T = typename decltype(tag)::type;
    return launch(maxpool2_bwd_kernel<T, true>, vgrid((long)N * H * W * (C / VW)), stream, dmp, dmpps, argmax, dsm,
        dsmps, dx, dxps, 0, N, H, W, C);
  });
}

