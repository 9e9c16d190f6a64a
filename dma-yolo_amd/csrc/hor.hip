// GnConv / HorBlock (models/common.py:1318-1400): the recursive gate product of GnConv.forward (:1349-1355) on channel
// slices of wider NHWC buffers, and HorBlock's layer-scaled residual x + gamma * f(x) (:1384-1398) with the gradient of
// gamma.
//
// All kernels are streaming passes over NHWC rows, bandwidth-bound: 16-byte loads and stores (C % 8 == 0 in bf16,
// C % 4 == 0 in fp32, 16-byte aligned bases and pixel strides), fp32 arithmetic, one rounding to storage per output
// element, no atomics.  Every strided tensor has its own pixel stride, so an operand may be a channel slice of a wider
// buffer (pwa / abc of fused_x, dw_list[i] of dw_abc, and their gradients).  Anything else returns
// hipErrorInvalidValue and launches nothing.
//
// The elementwise passes run one thread per 16-byte vector of the [M][C / VW] index space (a gate slice may be one
// vector wide, so a thread-per-channel-vector row walk would leave most of a block idle).  The layer-scale backward
// keeps bn.hip's row walk instead: a thread owns one channel vector, so its share of sum_m dout * y stays in registers;
// the block's row groups are summed through LDS in a fixed order into one partial row per block, and dmy_reduce_rows
// sums the rows in row order: bit-identical run to run.
#include "launch.h"

namespace {

// vector index over [M][CV] -> (row, first channel); 32-bit division whenever the index fits
DEV long vec_row(long i, int CV, int VW, int& c) {
  if ((unsigned long)i < 0xFFFFFFFFul) {
    const unsigned u = (unsigned)i, m = u / (unsigned)CV;
    c = (int)(u - m * (unsigned)CV) * VW;
    return (long)m;
  }
  const long m = i / CV;
  c = (int)(i - m * CV) * VW;
  return m;
}

// -------- y = a * b * scale
template <typename T>
__global__ void __launch_bounds__(256) gate_fwd_kernel(const T* __restrict__ a, long aps, const T* __restrict__ b,
                                                       long bps, T* __restrict__ y, long yps, long M, int C,
                                                       float scale) {
  constexpr int VW = Traits<T>::VW;
  const int CV = C / VW;
  const long total = M * CV;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    int c;
    const long m = vec_row(i, CV, VW, c);
    const uint4 av = *reinterpret_cast<const uint4*>(a + m * aps + c);
    const uint4 bv = *reinterpret_cast<const uint4*>(b + m * bps + c);
    float af[VW], bf[VW];
    unpack<T>(av, af);
    unpack<T>(bv, bf);
#pragma unroll
    for (int j = 0; j < VW; ++j) af[j] = af[j] * bf[j] * scale;
    *reinterpret_cast<uint4*>(y + m * yps + c) = pack<T>(af);
  }
}

// -------- da = dy * b * scale, db = dy * a * scale
template <typename T>
__global__ void __launch_bounds__(256) gate_bwd_kernel(const T* __restrict__ dy, long dps, const T* __restrict__ a,
                                                       long aps, const T* __restrict__ b, long bps,
                                                       T* __restrict__ da, long daps, T* __restrict__ db, long dbps,
                                                       long M, int C, float scale) {
  constexpr int VW = Traits<T>::VW;
  const int CV = C / VW;
  const long total = M * CV;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    int c;
    const long m = vec_row(i, CV, VW, c);
    const uint4 gv = *reinterpret_cast<const uint4*>(dy + m * dps + c);
    const uint4 av = *reinterpret_cast<const uint4*>(a + m * aps + c);
    const uint4 bv = *reinterpret_cast<const uint4*>(b + m * bps + c);
    float gf[VW], af[VW], bf[VW];
    unpack<T>(gv, gf);
    unpack<T>(av, af);
    unpack<T>(bv, bf);
#pragma unroll
    for (int j = 0; j < VW; ++j) {
      const float ga = gf[j] * bf[j] * scale, gb = gf[j] * af[j] * scale;
      af[j] = ga;
      bf[j] = gb;
    }
    *reinterpret_cast<uint4*>(da + m * daps + c) = pack<T>(af);
    *reinterpret_cast<uint4*>(db + m * dbps + c) = pack<T>(bf);
  }
}

// -------- out = x + gamma[c] * y (y dense)
template <typename T>
__global__ void __launch_bounds__(256) layerscale_fwd_kernel(const T* __restrict__ x, long xps, const T* __restrict__ y,
                                                             const float* __restrict__ gamma, T* __restrict__ out,
                                                             long ops, long M, int C) {
  constexpr int VW = Traits<T>::VW;
  const int CV = C / VW;
  const long total = M * CV;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    int c;
    const long m = vec_row(i, CV, VW, c);
    const uint4 xv = *reinterpret_cast<const uint4*>(x + m * xps + c);
    const uint4 yv = *reinterpret_cast<const uint4*>(y + m * C + c);
    float xf[VW], yf[VW], g[VW];
    ldf<VW>(gamma + c, g);
    unpack<T>(xv, xf);
    unpack<T>(yv, yf);
#pragma unroll
    for (int j = 0; j < VW; ++j) xf[j] = xf[j] + g[j] * yf[j];
    *reinterpret_cast<uint4*>(out + m * ops + c) = pack<T>(xf);
  }
}

// -------- dy = gamma[c] * dout (dense), part[block][c] = sum over the block's rows of dout * y.  bn.hip's thread
// mapping: 256 threads cover RB rows x CV channel vectors, rows grid-strided in increasing order
template <typename T>
__global__ void __launch_bounds__(256) layerscale_bwd_kernel(const T* __restrict__ dout, long dps,
                                                             const T* __restrict__ y, const float* __restrict__ gamma,
                                                             T* __restrict__ dy, long M, int C,
                                                             float* __restrict__ part) {
  constexpr int VW = Traits<T>::VW;
  __shared__ float red[256 * VW];
  const int CV = C / VW, RB = 256 / CV;
  const int cv = threadIdx.x % CV, rr = threadIdx.x / CV, c0 = cv * VW;
  float s[VW];
#pragma unroll
  for (int j = 0; j < VW; ++j) s[j] = 0.f;
  if (rr < RB) {
    float g[VW];
    ldf<VW>(gamma + c0, g);
    const long S = (long)gridDim.x * RB;
    for (long m = (long)blockIdx.x * RB + rr; m < M; m += S) {
      const uint4 gv = *reinterpret_cast<const uint4*>(dout + m * dps + c0);
      const uint4 yv = *reinterpret_cast<const uint4*>(y + m * C + c0);
      float gf[VW], yf[VW];
      unpack<T>(gv, gf);
      unpack<T>(yv, yf);
#pragma unroll
      for (int j = 0; j < VW; ++j) {
        s[j] += gf[j] * yf[j];
        gf[j] = g[j] * gf[j];
      }
      *reinterpret_cast<uint4*>(dy + m * C + c0) = pack<T>(gf);
    }
  }
#pragma unroll
  for (int j = 0; j < VW; ++j) red[threadIdx.x * VW + j] = s[j];
  __syncthreads();
  // one thread per channel sums the RB row groups in order
  for (int c = threadIdx.x; c < C; c += blockDim.x) {
    const int v = c / VW, j = c % VW;
    float t = 0.f;
    for (int r = 0; r < RB; ++r) t += red[(r * CV + v) * VW + j];
    part[(long)blockIdx.x * C + c] = t;
  }
}

}  // namespace

DMY_API int dmy_gate_fwd(int dtype, const void* a, long aps, const void* b, long bps, void* y, long yps, long M, int C,
                         float scale, void* stream) {
  const int VW = vec_width(dtype);
  if (M < 1 || C < VW || !vec_ok(VW, C, {aps, bps, yps}, {a, b, y}) || !rows_fit(C, {aps, bps, yps}))
    return kInvalid;
  return by_dtype(dtype, kInvalid, [&](auto tag) {
    using T = typename decltype(tag)::type;
    return launch(gate_fwd_kernel<T>, vgrid(M * (C / VW)), stream, a, aps, b, bps, y, yps, M, C, scale);
  });
}

DMY_API int dmy_gate_bwd(int dtype, const void* dy, long dps, const void* a, long aps, const void* b, long bps, void* da,
                         long daps, void* db, long dbps, long M, int C, float scale, void* stream) {
  const int VW = vec_width(dtype);
  if (M < 1 || C < VW || !vec_ok(VW, C, {dps, aps, bps, daps, dbps}, {dy, a, b, da, db}) ||
      !rows_fit(C, {dps, aps, bps, daps, dbps}))
    return kInvalid;
  return by_dtype(dtype, kInvalid, [&](auto tag) {
    using T = typename decltype(tag)::type;
    return launch(gate_bwd_kernel<T>, vgrid(M * (C / VW)), stream, dy, dps, a, aps, b, bps, da, daps, db, dbps, M, C,
        scale);
  });
}

DMY_API int dmy_layerscale_fwd(int dtype, const void* x, long xps, const void* y, const float* gamma, void* out,
                               long ops, long M, int C, void* stream) {
  const int VW = vec_width(dtype);
  if (M < 1 || C < VW || !vec_ok(VW, C, {xps, ops}, {x, y, out}) || !rows_fit(C, {xps, ops}) || !gamma)
    return kInvalid;
  return by_dtype(dtype, kInvalid, [&](auto tag) {
    using T = typename decltype(tag)::type;
    return launch(layerscale_fwd_kernel<T>, vgrid(M * (C / VW)), stream, x, xps, y, gamma, out, ops, M, C);
  });
}

// one partial row per block: a block per 32 rows, capped at 2048
DMY_API int dmy_layerscale_bwd_rows(long M) { return M < 1 ? 0 : grid_cap(ceil_div(M, 32), 2048); }

// a row is at most 256 vectors (the kernel's thread mapping)
DMY_API int dmy_layerscale_bwd(int dtype, const void* dout, long dps, const void* y, const float* gamma, void* dy,
                               long M, int C, float* part, void* stream) {
  const int VW = vec_width(dtype);
  if (M < 1 || C < VW || !vec_ok(VW, C, {dps}, {dout, y, dy}) || dps < C || C / VW > 256 || !gamma || !part)
    return kInvalid;
  return by_dtype(dtype, kInvalid, [&](auto tag) {
    using T = typename decltype(tag)::type;
    return launch(layerscale_bwd_kernel<T>, dmy_layerscale_bwd_rows(M), stream, dout, dps, y, gamma, dy, M, C, part);
  });
}

