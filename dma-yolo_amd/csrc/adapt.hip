// Adaptive-fusion necks: the per-pixel softmax gate of AdaptConcat (models/common.py:953-992) and the weighted add +
// SiLU of Adapt_Add2 / Adapt_Add3 (models/common.py:1028-1061), forward and backward.
//
// All four kernels are streaming passes over NHWC rows, bandwidth-bound: 16-byte loads and stores, fp32 arithmetic, one
// rounding to storage per output element, no atomics.  Every tensor has its own pixel stride, so inputs and gradient
// targets may be channel slices of wider buffers (concat buffers, GradSink buffers).
//
// Gate.  A pixel is owned by LP consecutive lanes (LP a power of two, 4..64, sized on the host from the channel count:
// one lane per 16-byte vector of the concatenated row, at least one per vector of the level-map row).  Lane j holds the
// columns of weight_levels that multiply vector j of the level maps wm [M][16 L]; the L logits are the xor-butterfly
// sum of the lanes' partial dot products (a + b == b + a, so every lane of the group ends with the same bits), the
// softmax runs redundantly per lane in fp32 with the maximum subtracted, and the lanes then stream the pixel's
// channels.  The backward accumulates the weight_levels / bias gradients in registers over the pixels a lane visits
// and reduces them across the block in a fixed order into one partial row per block; dmy_reduce_rows sums the rows in
// row order, so the result is bit-identical from run to run.
#include "launch.h"

namespace {

template <typename T> struct Levels {
  const T* x[3];   // inputs
  T* dx[3];        // input gradients (backward)
  long xps[3];     // pixel strides of x
  long dxps[3];    // pixel strides of dx
  int voff[4];     // first 16-byte vector of each level in the concatenated row; voff[L] = vectors per row
};

template <typename T> DEV int level_of(const Levels<T>& A, int v, int L) {
  return (L == 3 && v >= A.voff[2]) ? 2 : (v >= A.voff[1] ? 1 : 0);
}
DEV float pick(const float* a, int l) { return l == 0 ? a[0] : (l == 1 ? a[1] : a[2]); }

template <typename T, int L>
__global__ void __launch_bounds__(256)
adapt_gate_fwd_kernel(Levels<T> A, const T* __restrict__ wm, long wmps, const float* __restrict__ W,
                      const float* __restrict__ bias, T* __restrict__ y, long yps, float* __restrict__ a, long M,
                      int lpshift) {
  constexpr int VW = Traits<T>::VW, NW = 16 * L, NWV = NW / VW;
  const int LP = 1 << lpshift, j = threadIdx.x & (LP - 1), nv = A.voff[L];
  const long gpb = 256 >> lpshift;
  float wr[L][VW];
#pragma unroll
  for (int l = 0; l < L; ++l)
#pragma unroll
    for (int e = 0; e < VW; ++e) wr[l][e] = j < NWV ? W[l * NW + j * VW + e] : 0.f;
  float bl[3] = {0.f, 0.f, 0.f};
#pragma unroll
  for (int l = 0; l < L; ++l) bl[l] = bias[l];
  for (long base = blockIdx.x * gpb; base < M; base += (long)gridDim.x * gpb) {
    const long m = base + (threadIdx.x >> lpshift);
    const bool valid = m < M;
    float lg[3] = {0.f, 0.f, 0.f};
    if (valid && j < NWV) {
      float f[VW];
      unpack<T>(*reinterpret_cast<const uint4*>(wm + m * wmps + j * VW), f);
#pragma unroll
      for (int l = 0; l < L; ++l)
#pragma unroll
        for (int e = 0; e < VW; ++e) lg[l] += wr[l][e] * f[e];
    }
    for (int o = LP >> 1; o > 0; o >>= 1) {
#pragma unroll
      for (int l = 0; l < L; ++l) lg[l] += __shfl_xor(lg[l], o, 64);
    }
    float mx = -INFINITY, s = 0.f;
#pragma unroll
    for (int l = 0; l < L; ++l) {
      lg[l] += bl[l];
      mx = fmaxf(mx, lg[l]);
    }
#pragma unroll
    for (int l = 0; l < L; ++l) {
      lg[l] = __expf(lg[l] - mx);
      s += lg[l];
    }
    const float inv = 1.0f / s;
#pragma unroll
    for (int l = 0; l < L; ++l) lg[l] *= inv;
    if (!valid) continue;
    if (j == 0) {
#pragma unroll
      for (int l = 0; l < L; ++l) a[m * L + l] = lg[l];
    }
    for (int v = j; v < nv; v += LP) {
      const int l = level_of(A, v, L);
      const float al = pick(lg, l);
      float f[VW];
      unpack<T>(*reinterpret_cast<const uint4*>(A.x[l] + m * A.xps[l] + (long)(v - A.voff[l]) * VW), f);
#pragma unroll
      for (int e = 0; e < VW; ++e) f[e] *= al;
      *reinterpret_cast<uint4*>(y + m * yps + (long)v * VW) = pack<T>(f);
    }
  }
}

// accumulate: bit l set -> dx_l += (a GradSink that already holds a contribution)
template <typename T, int L>
__global__ void __launch_bounds__(256)
adapt_gate_bwd_kernel(Levels<T> A, const T* __restrict__ dy, long dps, const float* __restrict__ a,
                      const T* __restrict__ wm, long wmps, const float* __restrict__ W, int accumulate,
                      T* __restrict__ dwm, long dwmps, float* __restrict__ pdw, float* __restrict__ pdb, long M,
                      int lpshift) {
  constexpr int VW = Traits<T>::VW, NW = 16 * L, NWV = NW / VW;
  const int LP = 1 << lpshift, j = threadIdx.x & (LP - 1), nv = A.voff[L];
  const long gpb = 256 >> lpshift;
  float wr[L][VW], acc[L][VW], accb[L];
#pragma unroll
  for (int l = 0; l < L; ++l) {
    accb[l] = 0.f;
#pragma unroll
    for (int e = 0; e < VW; ++e) {
      wr[l][e] = j < NWV ? W[l * NW + j * VW + e] : 0.f;
      acc[l][e] = 0.f;
    }
  }
  for (long base = blockIdx.x * gpb; base < M; base += (long)gridDim.x * gpb) {
    const long m = base + (threadIdx.x >> lpshift);
    const bool valid = m < M;
    float al[3] = {0.f, 0.f, 0.f}, da[3] = {0.f, 0.f, 0.f};
    if (valid) {
#pragma unroll
      for (int l = 0; l < L; ++l) al[l] = a[m * L + l];
      for (int v = j; v < nv; v += LP) {
        const int l = level_of(A, v, L);
        const long c = (long)(v - A.voff[l]) * VW;
        const float sc = pick(al, l);
        float g[VW], xv[VW];
        unpack<T>(*reinterpret_cast<const uint4*>(dy + m * dps + (long)v * VW), g);
        unpack<T>(*reinterpret_cast<const uint4*>(A.x[l] + m * A.xps[l] + c), xv);
        float d = 0.f;
#pragma unroll
        for (int e = 0; e < VW; ++e) d += g[e] * xv[e];
        if (l == 0) da[0] += d;
        else if (l == 1) da[1] += d;
        else da[2] += d;
        T* dst = A.dx[l] + m * A.dxps[l] + c;
        if ((accumulate >> l) & 1) {
          float o[VW];
          unpack<T>(*reinterpret_cast<const uint4*>(dst), o);
#pragma unroll
          for (int e = 0; e < VW; ++e) g[e] = g[e] * sc + o[e];
        } else {
#pragma unroll
          for (int e = 0; e < VW; ++e) g[e] *= sc;
        }
        *reinterpret_cast<uint4*>(dst) = pack<T>(g);
      }
    }
    for (int o = LP >> 1; o > 0; o >>= 1) {
#pragma unroll
      for (int l = 0; l < L; ++l) da[l] += __shfl_xor(da[l], o, 64);
    }
    float dot = 0.f, dl[L];
#pragma unroll
    for (int l = 0; l < L; ++l) dot += al[l] * da[l];
#pragma unroll
    for (int l = 0; l < L; ++l) dl[l] = al[l] * (da[l] - dot);  // 0 for a pixel past the end (al == 0)
    if (valid && j < NWV) {
      float f[VW], d[VW];
      unpack<T>(*reinterpret_cast<const uint4*>(wm + m * wmps + j * VW), f);
#pragma unroll
      for (int e = 0; e < VW; ++e) d[e] = 0.f;
#pragma unroll
      for (int l = 0; l < L; ++l)
#pragma unroll
        for (int e = 0; e < VW; ++e) {
          d[e] += wr[l][e] * dl[l];
          acc[l][e] += dl[l] * f[e];
        }
      *reinterpret_cast<uint4*>(dwm + m * dwmps + j * VW) = pack<T>(d);
      if (j == 0) {
#pragma unroll
        for (int l = 0; l < L; ++l) accb[l] += dl[l];
      }
    }
  }
  // block reduction in a fixed order: the groups of a wave (butterfly over the lane bits above LP), then the 4 waves
  __shared__ float red[4][NWV][L * VW];
  __shared__ float redb[4][L];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int l = 0; l < L; ++l) {
    for (int o = LP; o < 64; o <<= 1) accb[l] += __shfl_xor(accb[l], o, 64);
#pragma unroll
    for (int e = 0; e < VW; ++e) {
      for (int o = LP; o < 64; o <<= 1) acc[l][e] += __shfl_xor(acc[l][e], o, 64);
    }
  }
  if (lane < NWV && lane < LP) {
#pragma unroll
    for (int l = 0; l < L; ++l)
#pragma unroll
      for (int e = 0; e < VW; ++e) red[wave][lane][l * VW + e] = acc[l][e];
  }
  if (lane == 0) {
#pragma unroll
    for (int l = 0; l < L; ++l) redb[wave][l] = accb[l];
  }
  __syncthreads();
  const int t = threadIdx.x;
  if (t < L * NW) {
    const int l = t / NW, k = t % NW, jj = k / VW, e = k % VW;
    pdw[(long)blockIdx.x * (L * NW) + t] =
        ((red[0][jj][l * VW + e] + red[1][jj][l * VW + e]) + red[2][jj][l * VW + e]) + red[3][jj][l * VW + e];
  }
  if (t < L) pdb[(long)blockIdx.x * L + t] = ((redb[0][t] + redb[1][t]) + redb[2][t]) + redb[3][t];
}

// ---------------------------------------------------------------- weighted add + SiLU
struct AddW {
  float wn[3];
};
DEV AddW add_weights(const float* w, int n, float eps) {
  float s = eps;
  for (int i = 0; i < n; ++i) s += w[i];
  AddW r;
  for (int i = 0; i < 3; ++i) r.wn[i] = i < n ? w[i] / s : 0.f;
  return r;
}

template <typename T, int NI>
__global__ void __launch_bounds__(256)
adapt_add_fwd_kernel(Levels<T> A, const float* __restrict__ w, float eps, T* __restrict__ y, long yps, long M, int C) {
  constexpr int VW = Traits<T>::VW;
  const AddW wn = add_weights(w, NI, eps);
  const int cv = C / VW;
  const long total = M * cv;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long m = i / cv;
    const long c = (i - m * cv) * VW;
    float s[VW];
#pragma unroll
    for (int e = 0; e < VW; ++e) s[e] = 0.f;
#pragma unroll
    for (int k = 0; k < NI; ++k) {
      float f[VW];
      unpack<T>(*reinterpret_cast<const uint4*>(A.x[k] + m * A.xps[k] + c), f);
#pragma unroll
      for (int e = 0; e < VW; ++e) s[e] += wn.wn[k] * f[e];
    }
    act_fwd_n<VW>(ACT_SILU, s);
    *reinterpret_cast<uint4*>(y + m * yps + c) = pack<T>(s);
  }
}

// dx_k (+)= wn_k * dy * silu'(s), s recomputed from the saved inputs; part[k * gridDim.x + block] = the block's share of
// sum(dy * silu'(s) * x_k), the layout dmy_bifpn_wgrad reads
template <typename T, int NI>
__global__ void __launch_bounds__(256)
adapt_add_bwd_kernel(Levels<T> A, const T* __restrict__ dy, long dps, const float* __restrict__ w, float eps,
                     int accumulate, float* __restrict__ part, long M, int C) {
  constexpr int VW = Traits<T>::VW;
  const AddW wn = add_weights(w, NI, eps);
  const int cv = C / VW;
  const long total = M * cv;
  float dot[NI];
#pragma unroll
  for (int k = 0; k < NI; ++k) dot[k] = 0.f;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long m = i / cv;
    const long c = (i - m * cv) * VW;
    float s[VW], xv[NI][VW], g[VW];
#pragma unroll
    for (int e = 0; e < VW; ++e) s[e] = 0.f;
#pragma unroll
    for (int k = 0; k < NI; ++k) {
      unpack<T>(*reinterpret_cast<const uint4*>(A.x[k] + m * A.xps[k] + c), xv[k]);
#pragma unroll
      for (int e = 0; e < VW; ++e) s[e] += wn.wn[k] * xv[k][e];
    }
    act_grad_n<VW>(ACT_SILU, s);
    unpack<T>(*reinterpret_cast<const uint4*>(dy + m * dps + c), g);
#pragma unroll
    for (int e = 0; e < VW; ++e) g[e] *= s[e];
#pragma unroll
    for (int k = 0; k < NI; ++k) {
      float o[VW];
      T* dst = A.dx[k] + m * A.dxps[k] + c;
      if ((accumulate >> k) & 1) {
        unpack<T>(*reinterpret_cast<const uint4*>(dst), o);
#pragma unroll
        for (int e = 0; e < VW; ++e) o[e] += wn.wn[k] * g[e];
      } else {
#pragma unroll
        for (int e = 0; e < VW; ++e) o[e] = wn.wn[k] * g[e];
      }
      *reinterpret_cast<uint4*>(dst) = pack<T>(o);
#pragma unroll
      for (int e = 0; e < VW; ++e) dot[k] += g[e] * xv[k][e];
    }
  }
  __shared__ float red[NI][4];
#pragma unroll
  for (int k = 0; k < NI; ++k) {
    const float v = wave_sum(dot[k]);
    if ((threadIdx.x & 63) == 0) red[k][threadIdx.x >> 6] = v;
  }
  __syncthreads();
  if (threadIdx.x < NI)
    part[(long)threadIdx.x * gridDim.x + blockIdx.x] =
        ((red[threadIdx.x][0] + red[threadIdx.x][1]) + red[threadIdx.x][2]) + red[threadIdx.x][3];
}

// lanes per pixel (log2): one per 16-byte vector of the concatenated row, at least one per level-map vector
inline int gate_lpshift(int dtype, int Ct, int L) {
  const int VW = dtype ? 8 : 4, need = Ct / VW > 16 * L / VW ? Ct / VW : 16 * L / VW;
  int sh = 2;
  while ((1 << sh) < need && sh < 6) ++sh;
  return sh;
}

template <typename T>
bool fill_levels(Levels<T>& A, int n, const void* const* x, const long* xps, const int* C, void* const* dx,
                 const long* dxps) {
  constexpr int VW = Traits<T>::VW;
  int off = 0;
  for (int l = 0; l < 3; ++l) {
    const bool on = l < n;
    A.x[l] = on ? (const T*)x[l] : nullptr;
    A.dx[l] = on && dx ? (T*)dx[l] : nullptr;
    A.xps[l] = on ? xps[l] : 0;
    A.dxps[l] = on && dx ? dxps[l] : 0;
    A.voff[l] = off;
    if (!on) continue;
    if (C[l] <= 0 || !vec_ok(VW, C[l], {xps[l]}, {x[l]}) || xps[l] < C[l]) return false;
    if (dx && (!vec_ok(VW, C[l], {dxps[l]}, {dx[l]}) || dxps[l] < C[l])) return false;
    off += C[l] / VW;
  }
  for (int l = n; l <= 3; ++l) A.voff[l] = off;
  return true;
}

}  // namespace

DMY_API int dmy_adapt_gate_blocks(int dtype, long M, int Ct, int L) {
  const long gpb = 256 >> gate_lpshift(dtype, Ct, L);
  return grid_cap(ceil_div(M, gpb * 4), 2048);
}

DMY_API int dmy_adapt_gate_fwd(int dtype, int L, const void* x0, long x0ps, int C0, const void* x1, long x1ps, int C1,
                               const void* x2, long x2ps, int C2, const void* wm, long wmps, const float* W,
                               const float* b, void* y, long yps, float* a, long M, void* stream) {
  const int VW = vec_width(dtype), Ct = C0 + C1 + (L == 3 ? C2 : 0);
  if (L < 2 || L > 3 || M < 1 || !vec_ok(VW, Ct, {wmps, yps}, {wm, y}) || wmps < 16 * L || yps < Ct || !W || !b || !a)
    return -1;
  const void* xs[3] = {x0, x1, x2};
  const long xps[3] = {x0ps, x1ps, x2ps};
  const int Cs[3] = {C0, C1, C2};
  const int sh = gate_lpshift(dtype, Ct, L), grid = dmy_adapt_gate_blocks(dtype, M, Ct, L);
  return by_dtype(dtype, -1, [&](auto tag) {
    using T = typename decltype(tag)::type;
    Levels<T> A;
    if (!fill_levels<T>(A, L, xs, xps, Cs, nullptr, nullptr)) return -1;
    auto go = [&](auto nl) { return launch(adapt_gate_fwd_kernel<T, decltype(nl)::value>, grid, stream, A, wm, wmps, W,
        b, y, yps, a, M, sh); };
    return L == 2 ? go(Int<2>{}) : go(Int<3>{});
  });
}

DMY_API int dmy_adapt_gate_bwd(int dtype, int L, const void* dy, long dps, const void* x0, long x0ps, int C0,
                               const void* x1, long x1ps, int C1, const void* x2, long x2ps, int C2, const float* a,
                               const void* wm, long wmps, const float* W, void* dx0, long dx0ps, void* dx1, long dx1ps,
                               void* dx2, long dx2ps, int accumulate, void* dwm, long dwmps, float* pdw, float* pdb,
                               long M, void* stream) {
  const int VW = vec_width(dtype), Ct = C0 + C1 + (L == 3 ? C2 : 0);
  if (L < 2 || L > 3 || M < 1 || !vec_ok(VW, Ct, {wmps, dps, dwmps}, {wm, dy, dwm}) || wmps < 16 * L || dps < Ct ||
      dwmps < 16 * L || !W || !a || !pdw || !pdb)
    return -1;
  const void* xs[3] = {x0, x1, x2};
  const long xps[3] = {x0ps, x1ps, x2ps};
  const int Cs[3] = {C0, C1, C2};
  void* const dxs[3] = {dx0, dx1, dx2};
  const long dxps[3] = {dx0ps, dx1ps, dx2ps};
  const int sh = gate_lpshift(dtype, Ct, L), grid = dmy_adapt_gate_blocks(dtype, M, Ct, L);
  return by_dtype(dtype, -1, [&](auto tag) {
    using T = typename decltype(tag)::type;
    Levels<T> A;
    if (!fill_levels<T>(A, L, xs, xps, Cs, dxs, dxps)) return -1;
    auto go = [&](auto nl) { return launch(adapt_gate_bwd_kernel<T, decltype(nl)::value>, grid, stream, A, dy, dps, a,
        wm, wmps, W, accumulate, dwm, dwmps, pdw, pdb, M, sh); };
    return L == 2 ? go(Int<2>{}) : go(Int<3>{});
  });
}

DMY_API int dmy_adapt_add_fwd(int dtype, int n, const void* x0, long x0ps, const void* x1, long x1ps, const void* x2,
                              long x2ps, const float* w, float eps, void* y, long yps, long M, int C, void* stream) {
  if (n < 2 || n > 3 || M < 1 || !w || !vec_ok(vec_width(dtype), C, {yps}, {y}) || yps < C) return -1;
  const void* xs[3] = {x0, x1, x2};
  const long xps[3] = {x0ps, x1ps, x2ps};
  const int Cs[3] = {C, C, C};
  const int grid = dmy_dot_partial_blocks(M, C);
  return by_dtype(dtype, -1, [&](auto tag) {
    using T = typename decltype(tag)::type;
    Levels<T> A;
    if (!fill_levels<T>(A, n, xs, xps, Cs, nullptr, nullptr)) return -1;
    auto go = [&](auto ni) { return launch(adapt_add_fwd_kernel<T, decltype(ni)::value>, grid, stream, A, w, eps, y,
        yps, M, C); };
    return n == 2 ? go(Int<2>{}) : go(Int<3>{});
  });
}

DMY_API int dmy_adapt_add_bwd(int dtype, int n, const void* dy, long dps, const void* x0, long x0ps, const void* x1,
                              long x1ps, const void* x2, long x2ps, const float* w, float eps, void* dx0, long dx0ps,
                              void* dx1, long dx1ps, void* dx2, long dx2ps, int accumulate, float* part, long M, int C,
                              void* stream) {
  if (n < 2 || n > 3 || M < 1 || !w || !part || !vec_ok(vec_width(dtype), C, {dps}, {dy}) || dps < C) return -1;
  const void* xs[3] = {x0, x1, x2};
  const long xps[3] = {x0ps, x1ps, x2ps};
  const int Cs[3] = {C, C, C};
  void* const dxs[3] = {dx0, dx1, dx2};
  const long dxps[3] = {dx0ps, dx1ps, dx2ps};
  const int grid = dmy_dot_partial_blocks(M, C);
  return by_dtype(dtype, -1, [&](auto tag) {
    using T = typename decltype(tag)::type;
    Levels<T> A;
    if (!fill_levels<T>(A, n, xs, xps, Cs, dxs, dxps)) return -1;
    auto go = [&](auto ni) { return launch(adapt_add_bwd_kernel<T, decltype(ni)::value>, grid, stream, A, dy, dps, w,
        eps, accumulate, part, M, C); };
    return n == 2 ? go(Int<2>{}) : go(Int<3>{});
  });
}

