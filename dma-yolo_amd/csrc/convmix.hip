// Activation BEFORE BatchNorm, NHWC: the four passes of conv(+bias) -> GELU -> BatchNorm2d, both halves of ConvMix
// (models/cspcm.py:28-37).  bn.hip computes act(z * scale + shift) with statistics over z; here the batch statistics are
// over a = act(z), the backward runs through the BN first and act' second, and the conv bias gets a real gradient (the
// column sums of dz, which the apply pass writes as partial rows in the same launch).  a is recomputed from the stored z
// in every pass and never written to memory.
//
// A thread owns one 16-byte channel vector; a block covers a tile of TC channel units (a power of two <= 32, blockIdx.y
// picks the tile) by 256 / TC pixels and walks the pixel groups with a grid stride, so any whole number of vectors is
// taken (no limit on C) and the number of partial rows is bounded.  Every load and store is predicated on its own pixel
// (m < M) and channel unit.  Reductions go lane -> wave (xor shuffles over the lanes that share a channel unit) -> block
// (the four waves through LDS, summed in wave order) -> one row per block: no atomics, run-to-run bit-identical.  The
// rows have the format of dmy_bn_stats ([dmy_bn_partial_rows(M)][C]), so dmy_bn_finalize, dmy_bn_bwd_finalize,
// dmy_colsum2 and dmy_reduce_rows finish them unchanged.
#include "launch.h"
#include "tile.h"

namespace {

// psum / psq: per-block sums of a = act(z) and a * a
template <typename T>
__global__ void __launch_bounds__(256)
actbn_stats_kernel(const T* __restrict__ z, long zps, int act, long M, int C, int tcl, float* __restrict__ psum,
                   float* __restrict__ psq) {
  constexpr int VW = Traits<T>::VW;
  const Tile t(tcl, C, VW);
  float s1[VW], s2[VW];
#pragma unroll
  for (int e = 0; e < VW; ++e) { s1[e] = 0.f; s2[e] = 0.f; }
  if (t.cok) {
    for (long m = (long)blockIdx.x * t.PIX + t.rr; m < M; m += (long)gridDim.x * t.PIX) {
      float a[VW];
      load_vec<T>(z + m * zps + t.c0, a);
      act_fwd_n<VW>(act, a);
#pragma unroll
      for (int e = 0; e < VW; ++e) { s1[e] += a[e]; s2[e] += a[e] * a[e]; }
    }
  }
  write_rows<VW>(s1, s2, tcl, C, psum, psq);
}

// y = act(z) * scale + shift (+ res)
template <typename T>
__global__ void __launch_bounds__(256)
actbn_fwd_kernel(const T* __restrict__ z, long zps, int act, const float* __restrict__ scale,
                 const float* __restrict__ shift, const T* __restrict__ res, long rps, T* __restrict__ y, long yps, long M,
                 int C, int tcl) {
  constexpr int VW = Traits<T>::VW;
  const Tile t(tcl, C, VW);
  if (!t.cok) return;
  float sc[VW], sh[VW];
  ldf<VW>(scale + t.c0, sc);
  ldf<VW>(shift + t.c0, sh);
  for (long m = (long)blockIdx.x * t.PIX + t.rr; m < M; m += (long)gridDim.x * t.PIX) {
    float a[VW];
    load_vec<T>(z + m * zps + t.c0, a);
    act_fwd_n<VW>(act, a);
#pragma unroll
    for (int e = 0; e < VW; ++e) a[e] = a[e] * sc[e] + sh[e];
    if (res) {
      float r[VW];
      load_vec<T>(res + m * rps + t.c0, r);
#pragma unroll
      for (int e = 0; e < VW; ++e) a[e] += r[e];
    }
    *reinterpret_cast<uint4*>(y + m * yps + t.c0) = pack<T>(a);
  }
}

// pdb / pdg: per-block sums of dy and dy * ahat, ahat = (act(z) - mean) * invstd
template <typename T>
__global__ void __launch_bounds__(256)
actbn_bwd_reduce_kernel(const T* __restrict__ z, long zps, const T* __restrict__ dy, long dps,
                        const float* __restrict__ mean, const float* __restrict__ invstd, int act, long M, int C, int tcl,
                        float* __restrict__ pdb, float* __restrict__ pdg) {
  constexpr int VW = Traits<T>::VW;
  const Tile t(tcl, C, VW);
  float s1[VW], s2[VW];
#pragma unroll
  for (int e = 0; e < VW; ++e) { s1[e] = 0.f; s2[e] = 0.f; }
  if (t.cok) {
    float mu[VW], is[VW];
    ldf<VW>(mean + t.c0, mu);
    ldf<VW>(invstd + t.c0, is);
    for (long m = (long)blockIdx.x * t.PIX + t.rr; m < M; m += (long)gridDim.x * t.PIX) {
      float a[VW], g[VW];
      load_vec<T>(z + m * zps + t.c0, a);
      load_vec<T>(dy + m * dps + t.c0, g);
      act_fwd_n<VW>(act, a);
#pragma unroll
      for (int e = 0; e < VW; ++e) {
        s1[e] += g[e];
        s2[e] += g[e] * ((a[e] - mu[e]) * is[e]);
      }
    }
  }
  write_rows<VW>(s1, s2, tcl, C, pdb, pdg);
}

// dz = act'(z) * (ca * dy + cb + cc * ahat); train-mode BN: (ca, cb, cc) from dmy_bn_bwd_finalize, i.e.
// scale * (dy - mean(dy) - ahat * mean(dy * ahat)); eval mode: ca = scale, cb = cc = 0.  pdz (nullable): per-block sums
// of dz, the conv bias gradient's partial rows
template <typename T>
__global__ void __launch_bounds__(256)
actbn_bwd_apply_kernel(const T* __restrict__ z, long zps, const T* __restrict__ dy, long dps,
                       const float* __restrict__ mean, const float* __restrict__ invstd, int act,
                       const float* __restrict__ ca, const float* __restrict__ cb, const float* __restrict__ cc,
                       T* __restrict__ dz, long dzps, long M, int C, int tcl, float* __restrict__ pdz) {
  constexpr int VW = Traits<T>::VW;
  const Tile t(tcl, C, VW);
  float s1[VW], s2[VW];
#pragma unroll
  for (int e = 0; e < VW; ++e) { s1[e] = 0.f; s2[e] = 0.f; }
  if (t.cok) {
    float k1[VW], k0[VW], k2[VW], mu[VW], is[VW];
    ldf<VW>(ca + t.c0, k1);
    ldf<VW>(cb + t.c0, k0);
    ldf<VW>(cc + t.c0, k2);
    ldf<VW>(mean + t.c0, mu);
    ldf<VW>(invstd + t.c0, is);
#pragma unroll
    for (int e = 0; e < VW; ++e) {  // ca * dy + cb + cc * (a - mean) * invstd = k1 * dy + k0 + k2 * a
      k2[e] = k2[e] * is[e];
      k0[e] = k0[e] - k2[e] * mu[e];
    }
    for (long m = (long)blockIdx.x * t.PIX + t.rr; m < M; m += (long)gridDim.x * t.PIX) {
      float u[VW], a[VW], g[VW];
      load_vec<T>(z + m * zps + t.c0, u);
      load_vec<T>(dy + m * dps + t.c0, g);
#pragma unroll
      for (int e = 0; e < VW; ++e) a[e] = u[e];
      act_fwd_n<VW>(act, a);
      act_grad_n<VW>(act, u);
#pragma unroll
      for (int e = 0; e < VW; ++e) {
        u[e] = u[e] * (k1[e] * g[e] + k0[e] + k2[e] * a[e]);
        s1[e] += u[e];
      }
      *reinterpret_cast<uint4*>(dz + m * dzps + t.c0) = pack<T>(u);
    }
  }
  if (pdz) write_rows<VW>(s1, s2, tcl, C, pdz, nullptr);  // block-uniform
}

}  // namespace

DMY_API int dmy_actbn_stats(int dtype, const void* z, long zps, int act, long M, int C, float* psum, float* psq,
                            void* stream) {
  const int VW = vec_width(dtype), tcl = tile_log2(C / VW);
  if (!vec_ok(VW, C, {zps}, {z}) || M < 1 || C < VW || !rows_fit(C, {zps}) || !psum || !psq) return -1;
  const dim3 grid = tile_grid(dmy_bn_partial_rows(M), C / VW, tcl);
  return by_dtype(dtype, -1, [&](auto tag) {
    using T = typename decltype(tag)::type;
    return launch(actbn_stats_kernel<T>, grid, stream, z, zps, act, M, C, tcl, psum, psq);
  });
}

DMY_API int dmy_actbn_fwd(int dtype, const void* z, long zps, int act, const float* scale, const float* shift,
                          const void* res, long rps, void* y, long yps, long M, int C, void* stream) {
  const int VW = vec_width(dtype), tcl = tile_log2(C / VW);
  if (!vec_ok(VW, C, {zps, yps, res ? rps : 0}, {z, y}, {res}) || M < 1 || C < VW || !rows_fit(C, {zps, yps, res ? rps : C}) ||
      !scale || !shift)
    return -1;
  const dim3 grid = tile_grid(grid_cap(ceil_div(M, (long)(256 >> tcl) * 4), kEwCap), C / VW, tcl);
  return by_dtype(dtype, -1, [&](auto tag) {
    using T = typename decltype(tag)::type;
    return launch(actbn_fwd_kernel<T>, grid, stream, z, zps, act, scale, shift, res, rps, y, yps, M, C, tcl);
  });
}

DMY_API int dmy_actbn_bwd_reduce(int dtype, const void* z, long zps, const void* dy, long dps, const float* mean,
                                 const float* invstd, int act, long M, int C, float* pdb, float* pdg, void* stream) {
  const int VW = vec_width(dtype), tcl = tile_log2(C / VW);
  if (!vec_ok(VW, C, {zps, dps}, {z, dy}) || M < 1 || C < VW || !rows_fit(C, {zps, dps}) || !mean || !invstd || !pdb || !pdg)
    return -1;
  const dim3 grid = tile_grid(dmy_bn_partial_rows(M), C / VW, tcl);
  return by_dtype(dtype, -1, [&](auto tag) {
    using T = typename decltype(tag)::type;
    return launch(actbn_bwd_reduce_kernel<T>, grid, stream, z, zps, dy, dps, mean, invstd, act, M, C, tcl, pdb, pdg);
  });
}

DMY_API int dmy_actbn_bwd_apply(int dtype, const void* z, long zps, const void* dy, long dps, const float* mean,
                                const float* invstd, int act, const float* ca, const float* cb, const float* cc, void* dz,
                                long dzps, long M, int C, float* pdz, void* stream) {
  const int VW = vec_width(dtype), tcl = tile_log2(C / VW);
  if (!vec_ok(VW, C, {zps, dps, dzps}, {z, dy, dz}) || M < 1 || C < VW || !rows_fit(C, {zps, dps, dzps}) || !mean || !invstd ||
      !ca || !cb || !cc)
    return -1;
  const dim3 grid = tile_grid(dmy_bn_partial_rows(M), C / VW, tcl);
  return by_dtype(dtype, -1, [&](auto tag) {
    using T = typename decltype(tag)::type;
    return launch(actbn_bwd_apply_kernel<T>, grid, stream, z, zps, dy, dps, mean, invstd, act, ca, cb, cc, dz, dzps, M,
        C, tcl, pdz);
  });
}

